"""Surface queries on the CPU (rt_resolve_hits / rt_debug_resolve_host, csrc/rt_surface.h): the
record layouts, the host resolve against the oracle's G-buffer and against a numpy restatement from
the scene descriptor, degenerate normals and out-of-range triangle ids.  Every comparison is
bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surface_ref as sr
from conftest import ROOT
from helpers import textured_scene
from test_gpu_query import _DescScene, _batch, _desc_with

MISS = sr.MISS


# ---- 1. layouts ---------------------------------------------------------------------------------------
def test_surface_struct_layouts_match_c(rt, tmp_path):
    A = rt._abi
    sf = [n for n, _ in A.Surface._fields_]
    mf = [n for n, _ in A.SurfaceMaterial._fields_]
    lines = ["P(rt_surface); P(rt_surface_material);"]
    lines += [f"O(rt_surface, {f});" for f in sf] + [f"O(rt_surface_material, {f});" for f in mf]
    prog = tmp_path / "slayout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  ''' + "\n  ".join(lines) + r'''
  printf("flags %u %u %u %u\n", RT_SURFACE_HAS_UV, RT_SURFACE_BACKFACE, RT_SURFACE_NORMAL_MAPPED, RT_SURFACE_TRANSMISSIVE);
  return 0;
}''')
    exe = tmp_path / "slayout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    text = subprocess.check_output([str(exe)]).decode().splitlines()
    out = dict(line.rsplit(" ", 1) for line in text if not line.startswith("flags"))
    assert int(out["rt_surface"]) == C.sizeof(A.Surface) == 64
    assert int(out["rt_surface_material"]) == C.sizeof(A.SurfaceMaterial) == 48
    for name, cls, fields in (("rt_surface", A.Surface, sf), ("rt_surface_material", A.SurfaceMaterial, mf)):
        for f in fields:
            assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    # the 16-B words
    assert [getattr(A.Surface, f).offset for f in ("position", "t", "normal", "u", "shading_normal", "v", "triangle",
                                                    "flags")] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert [getattr(A.SurfaceMaterial, f).offset for f in ("base_color", "opacity", "emission", "ior", "roughness",
                                                            "metallic", "texture_flags", "slot")] == [0, 12, 16, 28, 32, 36, 40, 44]
    assert [l for l in text if l.startswith("flags")] == ["flags 1 2 4 8"]
    assert (A.RT_SURFACE_HAS_UV, A.RT_SURFACE_BACKFACE, A.RT_SURFACE_NORMAL_MAPPED, A.RT_SURFACE_TRANSMISSIVE) == (1, 2, 4, 8)


def test_surface_null_arguments_return_status(rt):
    lib = rt.lib()
    E = rt._abi.RT_ERR_INVALID_ARG
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert lib.rt_resolve_hits(None, None, None, 0, None, None) == E
    assert lib.rt_resolve_hits(None, p, p, 1, p, p) == E
    assert lib.rt_resolve_hits_on(None, p, p, 1, p, None, None) == E
    assert lib.rt_debug_resolve_host(None, p, p, 1, p, p) == E
    assert lib.rt_last_error(None)   # message set, no crash


# ---- 2. host resolve against the oracle's G-buffer ------------------------------------------------------
def test_host_resolve_matches_oracle_gbuffer(rt, orc, assets):
    """Sample 0's primary rays of frame 0, traced and resolved on the host, against the G-buffer
    planes the oracle writes for that frame: every pixel, normal-mapped surfaces included."""
    W, H, seed = 96, 64, 21
    sc = textured_scene(rt, assets)
    u = rt.uniforms_default(W, H, sc.light_count)
    u.camera = u.previousCamera = rt.camera_default(W, H)
    u.samplesPerPixel, u.maxBounces, u.enableDenoiseGBuffer, u.frameIndex = 1, 1, 1, 0
    gb = orc.OracleScene(sc.desc()).render(u, rt.random_offsets(seed, W, H), gbuffer=True)["gbuffer"].reshape(4, W * H, 4)
    o, d = sr.camera_rays(rt, orc, W, H, seed)
    ref = rt.debug_trace_host(sc, o, d)
    S = rt.debug_resolve_host(sc, rt.Renderer.make_rays(o, d), sr.hit_records(ref))
    hit = ref["id"] != MISS
    mapped = (S.flags & S.NORMAL_MAPPED) != 0
    print(f"G-buffer check: {hit.sum()} of {W * H} pixels hit, {mapped.sum()} normal-mapped")
    assert hit.sum() > 0 and mapped.sum() > 0 and (hit & ~mapped).sum() > 0
    assert not np.array_equal(S.shading_normal[mapped], S.normal[mapped])
    F = np.float32
    metal = S.metallic[:, None]
    want = [S.base_color * (F(1) - metal), F(0.04) + (S.base_color - F(0.04)) * metal,
            S.shading_normal * F(0.5) + F(0.5), np.minimum(np.maximum(S.roughness, F(0)), F(1))[:, None]]
    for plane, (w, cols) in enumerate(zip(want, (3, 3, 3, 1))):
        assert np.array_equal(sr.bits(w[hit]), sr.bits(gb[plane][hit, :cols])), plane
    assert np.all(gb[:, ~hit] == 0)


# ---- 3. numpy restatement from the descriptor -----------------------------------------------------------
_CASES = {}


def surface_case(rt, orc, assets, preset, n):
    """Scene, the ray batch _batch(5, n) of tests/test_gpu_query.py, its host hits, the host
    resolve of them (with and without materials) and the numpy restatement; computed once, shared
    with tests/test_gpu_surface.py, never modified."""
    key = (preset, n)
    if key not in _CASES:
        if preset == "textured_scene":
            sc = textured_scene(rt, assets)
        elif preset == "c1+train":
            sc = rt.Scene.preset("c1", assets)
            sc.add_model(os.path.join(assets, "train.obj"), (-0.3, 0.0, 0.4), scale=0.5)
        else:
            sc = rt.Scene.preset(preset, assets)
        o, d = _batch(5, n)
        ref = rt.debug_trace_host(sc, o, d)
        A = sr.SceneArrays(sc.desc())
        rays = rt.Renderer.make_rays(o, d)
        hits = sr.with_owners(sr.hit_records(ref), A)
        _CASES[key] = dict(scene=sc, o=o, d=d, ref=ref, arrays=A, rays=rays, hits=hits,
                           host=rt.debug_resolve_host(sc, rays, hits),
                           host_nomat=rt.debug_resolve_host(sc, rays, hits, material=False))
    return _CASES[key]


def assert_records_equal(got, want, fields=sr.FLOAT_FIELDS + sr.INT_FIELDS, rows=slice(None), what=""):
    for f in fields:
        g, w = getattr(got, f) if not isinstance(got, dict) else got[f], getattr(want, f) if not isinstance(want, dict) else want[f]
        g, w = np.asarray(g)[rows], np.asarray(w)
        assert g.dtype == w.dtype and np.array_equal(sr.bits(g), sr.bits(w)), (what, f)


@pytest.mark.parametrize("preset,n", [("c1", 3000), ("textured_scene", 2000), ("c3g", 600)])
def test_host_resolve_matches_numpy_restatement(rt, orc, assets, preset, n):
    c = surface_case(rt, orc, assets, preset, n)
    S, A, ref = c["host"], c["arrays"], c["ref"]
    hit = ref["id"] != MISS
    osc = orc.OracleScene(c["scene"].desc())
    want = sr.restate(A, osc, c["o"][hit], c["d"][hit], ref["t"][hit], ref["id"][hit], ref["u"][hit], ref["v"][hit])
    fl = want["flags"].view(np.uint32)
    mapped = (fl & sr.NORMAL_MAPPED) != 0
    print(f"{preset}: {hit.sum()} hits of {len(hit)}, {((fl & sr.BACKFACE) != 0).sum()} back faces, "
          f"{((fl & sr.HAS_UV) != 0).sum()} textured, {mapped.sum()} normal-mapped, "
          f"{((fl & sr.TRANSMISSIVE) != 0).sum()} transmissive")
    assert 0 < hit.sum() < len(hit)
    assert 0 < ((fl & sr.BACKFACE) != 0).sum() < hit.sum()
    if preset == "textured_scene":
        assert ((fl & sr.HAS_UV) != 0).any() and mapped.any()
        # the sphere without UVs (mesh 1): every vertex UV is zero, so it samples (0, 1)
        sphere = (want["mesh"] == 1) & ((fl & sr.HAS_UV) != 0)
        assert sphere.any() and np.all(S.uv[hit][sphere] == np.array([0.0, 1.0], np.float32))
    else:
        assert not (fl & sr.HAS_UV).any()
    if preset == "c3g":
        assert ((fl & sr.TRANSMISSIVE) != 0).any()
    fields = [f for f in sr.FLOAT_FIELDS + sr.INT_FIELDS if f != "shading_normal"]
    assert_records_equal(S, want, fields, rows=hit, what=preset)
    # the shading normal is the normal except where a normal map was applied (the G-buffer test's part)
    assert np.array_equal(sr.bits(S.shading_normal[hit][~mapped]), sr.bits(want["normal"][~mapped]))
    # misses: exactly the stated bytes
    assert np.array_equal(sr.bits(S.buffer[~hit]), np.broadcast_to(sr.MISS_SURFACE, (int((~hit).sum()), 16)))
    assert not sr.bits(S.material_buffer[~hit]).any()
    # without materials the surface records are the same
    assert c["host_nomat"].material_buffer is None
    assert np.array_equal(sr.bits(c["host_nomat"].buffer), sr.bits(S.buffer))


# ---- 4. degenerate normals ------------------------------------------------------------------------------
def test_zero_normals_give_minus_direction(rt, orc, assets):
    c = surface_case(rt, orc, assets, "c1", 3000)
    desc = c["scene"].desc()
    A = c["arrays"]
    zeros = np.zeros((desc.meshes[0].vertex_count, 4), np.float32)   # the floor is mesh 0
    S = rt.debug_resolve_host(_DescScene(_desc_with(rt, desc, 0, normals=zeros)), c["rays"], c["hits"])
    hit = c["ref"]["id"] != MISS
    floor = hit.copy()
    floor[hit] = A.mesh[c["ref"]["id"][hit].astype(np.int64)] == 0
    assert floor.any() and (hit & ~floor).any()
    assert np.array_equal(sr.bits(S.normal[floor]), sr.bits(-c["d"][floor]))
    assert np.array_equal(sr.bits(S.shading_normal[floor]), sr.bits(-c["d"][floor]))
    assert not (S.flags[floor] & S.BACKFACE).any()   # dot(d, -d) < 0
    # every other hit keeps its record
    rest = hit & ~floor
    assert np.array_equal(sr.bits(S.buffer[rest]), sr.bits(c["host"].buffer[rest]))


# ---- 5. out-of-range ids ---------------------------------------------------------------------------------
def test_edited_triangle_ids_are_misses(rt, orc, assets):
    c = surface_case(rt, orc, assets, "c1", 3000)
    h = c["hits"].copy()
    hi = h.view(np.uint32)
    hit = np.flatnonzero(c["ref"]["id"] != MISS)
    a, b = hit[::2], hit[1::2]
    hi[a, 3] = c["arrays"].ntris
    hi[b, 3] = 0xFFFFFFFE
    S = rt.debug_resolve_host(c["scene"], c["rays"], h)
    assert np.array_equal(sr.bits(S.buffer), np.broadcast_to(sr.MISS_SURFACE, S.buffer.shape))
    assert not sr.bits(S.material_buffer).any()


def test_out_of_range_ids_under_sanitizers():
    """tools/surface_host_check.sh: a stand-alone program resolves hit records whose triangle ids
    are the triangle count, 0xfffffffe and RT_MISS through rt_debug_resolve_host, built under
    AddressSanitizer + UBSan; any report aborts it."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "surface_host_check.sh")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "surface_host_check: ok" in r.stdout, r.stdout
