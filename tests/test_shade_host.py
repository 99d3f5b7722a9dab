"""Shading queries on the CPU (rt_shade_hits / rt_debug_shade_host, csrc/rt_scatter.h): the record
layouts, the renderer's path tracer re-assembled from the host hooks (trace -> resolve -> shade ->
trace_any + trace -> ...) against the independent oracle's render, the Halton dimension map and the
record rules.  Every comparison is bitwise.

The glass case is c1 + the glass teapot + one small near-black sphere (shade_ref.glass_scene): the
sphere is what ends paths on the throughput cut-off, which no c1 material reaches in 8 bounces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shade_ref as sh
import surface_ref as sr
from conftest import ROOT
from helpers import lights_scene, textured_scene

F = np.float32
SEED = 21
# name -> (scene, W, H, spp, max bounces, shading mode, compact); both loop forms appear
CASES = {
    "c1": ("c1", 48, 32, 2, 4, 0, True),
    "c1-legacy": ("c1", 48, 32, 2, 3, 1, False),
    "textured": ("textured", 48, 32, 1, 3, 0, True),
    "sun": (["sun"], 32, 24, 1, 2, 0, False),
    "spot": (["spot"], 32, 24, 1, 2, 0, True),
    "point": (["point"], 32, 24, 1, 2, 0, False),
    "area+area2+spot": (["area", "area2", "spot"], 32, 24, 1, 2, 0, True),
    "glass": ("glass", 48, 27, 2, 8, 0, True),
}
_RESULTS = {}


def make_scene(rt, assets, what):
    if what == "textured":
        return textured_scene(rt, assets)
    if what == "glass":
        return sh.glass_scene(rt, assets)
    if isinstance(what, list):
        return lights_scene(rt, assets, what)
    return rt.Scene.preset(what, assets)


def shade_case(rt, orc, assets, name):
    """The host loop of a case, run once: its frame and counts, and the inputs of every shade call
    it made (rays, surface, material and path buffers, concatenated over the iterations of every
    sample: paths at every bounce / step the case reaches; the carry-form cases include dead
    records).  Shared with tests/test_gpu_shade.py, never modified."""
    if name not in _RESULTS:
        what, W, H, spp, mb, mode, compact = CASES[name]
        sc = make_scene(rt, assets, what)
        B = sh.HostBackend(rt, sc, mode, mb)
        recs = []
        got = sh.render(B, rt, orc, W, H, SEED, spp, mb, compact,
                        record=lambda r, S, p: recs.append((r, S.buffer, S.material_buffer, p.buffer)))
        rays, surf, mat, paths = (np.ascontiguousarray(np.concatenate([x[k] for x in recs])) for k in range(4))
        _RESULTS[name] = dict(scene=sc, backend=B, frame=got, W=W, H=H, spp=spp, max_bounces=mb, mode=mode,
                              rays=rays, surface=rt.Surface(surf, surf.view(np.int32), mat, mat.view(np.int32)),
                              paths=paths, shaded=B.shade(rays, rt.Surface(surf, surf.view(np.int32), mat, mat.view(np.int32)),
                                                          paths))
    return _RESULTS[name]


def take(c, rows):
    """Rows of a case's records: (rays, Surface, path buffer)."""
    s, m = c["surface"].buffer[rows], c["surface"].material_buffer[rows]
    return c["rays"][rows], type(c["surface"])(s, s.view(np.int32), m, m.view(np.int32)), c["paths"][rows]


def same(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


def assert_shaded_equal(got, want, what=""):
    for f in ("next_rays", "shadow_rays", "contrib"):
        assert same(getattr(got, f), getattr(want, f)), (what, f)
    assert same(got.paths.buffer, want.paths.buffer), (what, "paths")


# ---- 1. layouts -----------------------------------------------------------------------------------------
def test_shade_struct_layouts_match_c(rt, tmp_path):
    A = rt._abi
    pf = [n for n, _ in A.Path._fields_]
    of = [n for n, _ in A.ShadeOpts._fields_]
    lines = ["P(rt_path); P(rt_shade_opts);"] + [f"O(rt_path, {f});" for f in pf] + [f"O(rt_shade_opts, {f});" for f in of]
    prog = tmp_path / "playout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  ''' + "\n  ".join(lines) + r'''
  printf("flags %u %u\n", RT_PATH_ALIVE, RT_PATH_SHADOW);
  return 0;
}''')
    exe = tmp_path / "playout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    text = subprocess.check_output([str(exe)]).decode().splitlines()
    out = dict(line.rsplit(" ", 1) for line in text if not line.startswith("flags"))
    assert int(out["rt_path"]) == C.sizeof(A.Path) == 48
    assert int(out["rt_shade_opts"]) == C.sizeof(A.ShadeOpts) == 32
    for name, cls, fields in (("rt_path", A.Path, pf), ("rt_shade_opts", A.ShadeOpts, of)):
        for f in fields:
            assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    # the three 16-B words
    assert [getattr(A.Path, f).offset for f in ("throughput", "sample", "radiance", "flags", "bounce", "step",
                                                 "transparency_passes", "reserved")] == [0, 12, 16, 28, 32, 36, 40, 44]
    assert [l for l in text if l.startswith("flags")] == ["flags 1 2"]
    assert (A.RT_PATH_ALIVE, A.RT_PATH_SHADOW) == (1, 2) == (rt.Paths.ALIVE, rt.Paths.SHADOW)


def test_make_paths_host_layout(rt):
    p = rt.Renderer.make_paths(np.array([7, 2 ** 20 + 5], np.uint32))
    assert p.buffer.dtype == np.float32 and p.buffer.shape == (2, 12) and p.buffer.flags.c_contiguous
    rec = np.frombuffer(p.buffer.tobytes(), dtype=np.dtype(rt._abi.Path))
    assert rec["throughput"].tolist() == [[1, 1, 1], [1, 1, 1]] and not rec["radiance"].any()
    assert rec["sample"].tolist() == [7, 2 ** 20 + 5] and rec["flags"].tolist() == [1, 1]
    assert not (rec["bounce"].any() or rec["step"].any() or rec["transparency_passes"].any() or rec["reserved"].any())
    assert p.alive.all() and not p.shadow.any() and len(p) == 2


def test_shade_argument_errors_return_status(rt):
    """The checks rt_shade_hits and the host hook share, on the host hook; and the device entry
    points without a context."""
    A, L = rt._abi, rt.lib()
    E = A.RT_ERR_INVALID_ARG
    n = 4
    buf = np.zeros((6, n + 1, 16), F)   # rays, surfaces, materials, paths, next / shadow, contrib: 64 B a record is enough
    r, s, m, p, o, c = (buf[k].ctypes.data for k in range(6))
    nxt, sha = np.zeros((n, 8), F), np.zeros((n, 8), F)
    lights = (A.Light * 2)()
    lights[0].type = lights[1].type = 3

    def call(opts=(0, 2, 0), nl=2, lp=lights, **kw):
        a = dict(rays=r, surfaces=s, materials=m, randoms=None, n=n, paths=p, next_rays=nxt.ctypes.data,
                 shadow_rays=sha.ctypes.data, contrib=c)
        a.update(kw)
        op = None
        if opts is not None:
            op = A.ShadeOpts()
            op.shading_mode, op.max_bounces, op.light_count = opts
        return L.rt_debug_shade_host(lp, nl, C.byref(op) if op is not None else None, a["rays"], a["surfaces"], a["materials"],
                                     a["randoms"], a["n"], a["paths"], a["next_rays"], a["shadow_rays"], a["contrib"])

    assert call() == A.RT_OK   # all-zero records: dead paths
    assert call(opts=None) == E
    for name in ("rays", "surfaces", "materials", "paths", "next_rays", "shadow_rays", "contrib"):
        assert call(**{name: None}) == E, name
        assert call(**{name: dict(rays=r, surfaces=s, materials=m, paths=p, next_rays=nxt.ctypes.data,
                                  shadow_rays=sha.ctypes.data, contrib=c)[name] + 8}) == E, name
        assert call(**{name: dict(rays=r, surfaces=s, materials=m, paths=p, next_rays=nxt.ctypes.data,
                                  shadow_rays=sha.ctypes.data, contrib=c)[name] + 16}, n=n - 1) == A.RT_OK, name
    assert call(randoms=o) == A.RT_OK and call(randoms=o + 4) == E
    for bad in ((2, 2, 0), (-1, 2, 0), (0, 0, 0), (0, 13, 0), (0, 2, -1), (0, 2, 3)):
        assert call(opts=bad) == E, bad
    assert call(opts=(1, 12, 2)) == A.RT_OK
    assert call(nl=0) == E and call(nl=0, lp=None) == E   # an effective light count of 0
    assert call(n=0, rays=None, surfaces=None, materials=None, paths=None, next_rays=None, shadow_rays=None,
                contrib=None) == A.RT_OK
    assert call(n=0, opts=None) == E
    # the device entry points answer a NULL context with a status
    op = A.ShadeOpts(0, 2, 0)
    assert L.rt_shade_hits(None, C.byref(op), r, s, m, None, n, p, nxt.ctypes.data, sha.ctypes.data, c) == E
    assert L.rt_shade_hits_on(None, C.byref(op), r, s, m, None, 0, p, nxt.ctypes.data, sha.ctypes.data, c, None) == E
    assert L.rt_last_error(None)


# ---- 2. the host loop against the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_loop_equals_oracle(rt, orc, assets, name):
    c = shade_case(rt, orc, assets, name)
    W, H = c["W"], c["H"]
    u = rt.uniforms_default(W, H, c["scene"].light_count)
    u.camera = u.previousCamera = rt.camera_default(W, H)
    u.samplesPerPixel, u.maxBounces, u.shadingMode, u.frameIndex = c["spp"], c["max_bounces"], c["mode"], 0
    ref = orc.OracleScene(c["scene"].desc()).render(u, rt.random_offsets(SEED, W, H))
    got = c["frame"]
    print(f"{name}: {got['closest_rays']} closest rays, {got['shadow_rays']} shadow rays, {got['paths']} paths, "
          f"{len(c['paths'])} shade records")
    assert (got["closest_rays"], got["shadow_rays"], got["paths"]) == (ref["closest_rays"], ref["shadow_rays"], ref["paths"])
    assert same(got["radiance"], ref["radiance"][..., :3])
    assert got["radiance"].any()
    if name == "glass":
        P, Q, S = rt.Paths(c["paths"], c["paths"].view(np.int32)), c["shaded"].paths, c["surface"]
        refracted = Q.transparency_passes > 0
        cut = P.alive & (S.triangle != -1) & ~Q.alive & (Q.bounce < c["max_bounces"])
        print(f"glass: {refracted.sum()} refractions, deepest step {Q.step.max()}, {cut.sum()} cut-off ends")
        assert refracted.any()        # some record refracts
        assert Q.step.max() >= 11     # Halton dimensions >= 64: past what the frame kernels stage in LDS
        assert cut.any()              # some path ends on the throughput cut-off


# ---- 3. the dimension map ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "area+area2+spot", "glass"])
def test_randoms_from_the_documented_dimensions(rt, orc, assets, name):
    """randoms = None against randoms filled from the oracle's Halton at the dimensions the header
    states (5-stride of the bounce included): bit-equal."""
    c = shade_case(rt, orc, assets, name)
    rows = slice(None, None, max(1, len(c["paths"]) // 1500))
    rays, S, paths = take(c, rows)
    P = rt.Paths(paths, paths.view(np.int32))
    rnd = np.zeros((len(paths), 8), F)
    for k, (i, step) in enumerate(zip(P.sample.tolist(), P.step.tolist())):
        rnd[k, 0:4] = [orc.halton(i, 2 + 6 * step + d) for d in (0, 1, 2, 5)]
        rnd[k, 4:6] = [orc.halton(i, 2 + 5 * step + 3), orc.halton(i, 2 + 5 * step + 4)]
    B = c["backend"]
    plain, given = B.shade(rays, S, paths), B.shade(rays, S, paths, randoms=rnd)
    assert_shaded_equal(given, plain, name)
    assert plain.paths.step.max() > 0 and plain.paths.alive.any() and plain.paths.shadow.any()
    # ... and the numbers matter: others give other rays
    other = B.shade(rays, S, paths, randoms=np.roll(rnd, 1, axis=0))
    assert not same(other.next_rays, plain.next_rays)


# ---- 4. the record rules ---------------------------------------------------------------------------------------
def test_dead_records_are_left_alone(rt, orc, assets):
    c = shade_case(rt, orc, assets, "c1")
    rays, S, paths = take(c, slice(0, 600))
    dead = paths.copy()
    di = dead.view(np.uint32)
    di[:, 7] &= ~np.uint32(sh.ALIVE)
    di[::2, 7] |= sh.SHADOW   # left over from an earlier step
    out = c["backend"].shade(rays, S, dead)
    want = dead.copy()
    want.view(np.uint32)[:, 7] &= ~np.uint32(sh.SHADOW)
    assert same(out.paths.buffer, want)
    for rec in (out.next_rays, out.shadow_rays):
        assert same(rec, np.broadcast_to(sh.ZERO_RAY, rec.shape))
    assert not sr.bits(out.contrib).any()
    # the carry-form loop meets them by itself
    cc = shade_case(rt, orc, assets, "c1-legacy")
    Pin = rt.Paths(cc["paths"], cc["paths"].view(np.int32))
    was_dead = ~Pin.alive
    assert was_dead.any() and same(cc["shaded"].paths.buffer[was_dead][:, :7], cc["paths"][was_dead][:, :7])
    assert same(cc["shaded"].next_rays[was_dead], np.broadcast_to(sh.ZERO_RAY, (int(was_dead.sum()), 8)))


def test_miss_and_last_bounce_only_clear_alive(rt, orc, assets):
    c = shade_case(rt, orc, assets, "c1")
    rays, S, paths = take(c, slice(0, 600))
    P = rt.Paths(paths, paths.view(np.int32))
    assert P.alive.all() and (S.triangle != -1).any()
    ms = np.broadcast_to(sr.MISS_SURFACE.view(F), S.buffer.shape).copy()
    miss = rt.Surface(ms, ms.view(np.int32), np.zeros_like(S.material_buffer), np.zeros_like(S.material_buffer).view(np.int32))
    last = paths.copy()
    last.view(np.int32)[:, 8] = c["max_bounces"]
    for what, out, given in (("miss", c["backend"].shade(rays, miss, paths), paths),
                             ("last bounce", c["backend"].shade(rays, S, last), last)):
        want = given.copy()
        want.view(np.uint32)[:, 7] &= ~np.uint32(sh.ALIVE)
        assert same(out.paths.buffer, want), what
        for rec in (out.next_rays, out.shadow_rays):
            assert same(rec, np.broadcast_to(sh.ZERO_RAY, rec.shape)), what
        assert not sr.bits(out.contrib).any(), what
    # the loop's own misses (a miss surface from rt_debug_resolve_host) behave the same
    own = (S.triangle == -1)
    if own.any():
        assert not c["shaded"].paths.alive[:600][own].any()


@pytest.mark.parametrize("name", ["c1", "spot", "glass"])
def test_steps_without_a_ray_are_zero_filled(rt, orc, assets, name):
    c = shade_case(rt, orc, assets, name)
    out, Pin = c["shaded"], rt.Paths(c["paths"], c["paths"].view(np.int32))
    shaded = Pin.alive & (c["surface"].triangle != -1)
    no_shadow, ended = shaded & ~out.paths.shadow, shaded & ~out.paths.alive
    print(f"{name}: {shaded.sum()} shaded, {no_shadow.sum()} without a shadow ray, {ended.sum()} ended")
    if name != "c1":
        assert no_shadow.any()   # outside the spot's cone; glass hits
    assert ended.any()
    zero = lambda k: np.broadcast_to(sh.ZERO_RAY, (int(k.sum()), 8))
    assert same(out.shadow_rays[no_shadow], zero(no_shadow)) and not sr.bits(out.contrib[no_shadow]).any()
    assert same(out.next_rays[ended], zero(ended))
    live, lit = out.paths.alive, out.paths.shadow
    assert np.all(np.isposinf(out.next_rays[live, 7])) and not sr.bits(out.next_rays[live, 3]).any()
    assert np.all(out.shadow_rays[lit, 7] > 0) and not sr.bits(out.contrib[lit, 3]).any()
    if name == "glass":   # a glass hit adds no emission and keeps its radiance
        glass = shaded & ((c["surface"].flags & rt.Surface.TRANSMISSIVE) != 0)
        assert glass.any() and not out.paths.shadow[glass].any()
        assert same(out.paths.radiance[glass], Pin.radiance[glass])


def test_caller_numbers_under_sanitizers():
    """tools/shade_host_check.sh: a stand-alone program shades records whose light numbers are
    negative, 1, 2, huge, infinite and NaN and whose step is far outside the renderer's through
    rt_debug_shade_host, built under AddressSanitizer + UBSan, every array exactly as long as it
    must be; any report aborts it."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "shade_host_check.sh")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "shade_host_check: ok" in r.stdout, r.stdout


def test_light_index_is_clamped(rt, orc, assets):
    """A caller's light numbers of -1, 1, 2 and NaN pick lights 0 / last / last / 0: each equals the
    same record shaded with an in-range number that picks that light."""
    c = shade_case(rt, orc, assets, "area+area2+spot")
    rays, S, paths = take(c, slice(0, 400))
    rnd = np.random.default_rng(3).random((len(paths), 8)).astype(F)
    rnd[:, 6:] = 0
    B = c["backend"]

    def shade_with(x):
        r = rnd.copy()
        r[:, 0] = x
        return B.shade(rays, S, paths, randoms=r)

    first, middle, last = shade_with(0.1), shade_with(0.5), shade_with(0.9)   # (int)(x * 3) = 0, 1, 2
    assert not same(first.shadow_rays, last.shadow_rays) and not same(first.shadow_rays, middle.shadow_rays)
    assert not same(middle.shadow_rays, last.shadow_rays)
    for x, want in ((-1.0, first), (1.0, last), (2.0, last), (np.nan, first), (-np.inf, first), (np.inf, last)):
        assert_shaded_equal(shade_with(x), want, x)
