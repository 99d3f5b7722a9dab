"""Path queries on CPU (include/rt_api.h: rt_camera_paths .. rt_average_samples): the two new record
layouts against the header compiled with gcc, the camera host hook (rt_debug_camera_paths_host:
camera_record of csrc/rt_paths.h, the code rq_camera runs, compiled for the host) against the
references the shading tests already use (shade_ref.sample_rays: the oracle's Halton numbers and
numpy float32 arithmetic; Renderer.make_paths), and the argument checks that need no device.
Every comparison is bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shade_ref as sh
import surface_ref as sr
from conftest import ROOT

F = np.float32
W, H, SEED = 7, 5, 5   # a width that is no power of two: px = pix % W, py = pix / W
NEW_SYMBOLS = ["rt_camera_paths", "rt_camera_paths_on", "rt_compact_paths", "rt_compact_paths_on", "rt_connect_paths",
               "rt_connect_paths_on", "rt_retire_paths", "rt_retire_paths_on", "rt_average_samples", "rt_average_samples_on",
               "rt_debug_camera_paths_host", "rt_debug_compact_paths_host"]


def same(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


def uniforms(rt, frame=0, spp=2):
    u = rt.uniforms_default(W, H)
    u.camera = rt.camera_default(W, H)
    u.frameIndex, u.samplesPerPixel = frame, spp
    return u


# ---- 1. layouts and symbols ----------------------------------------------------------------------------
def test_path_struct_layouts_match_c(rt, tmp_path):
    A = rt._abi
    structs = (("rt_camera_opts", A.CameraOpts, 32), ("rt_compact_stream", A.CompactStream, 24))
    lines = []
    for name, cls, _ in structs:
        lines.append(f"P({name});")
        lines += [f"O({name}, {f});" for f, _ in cls._fields_]
    prog = tmp_path / "playout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  ''' + "\n  ".join(lines) + r'''
  printf("rt_path.reserved %zu\n", offsetof(rt_path, reserved));
  return 0;
}''')
    exe = tmp_path / "playout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, cls, size in structs:
        assert int(out[name]) == C.sizeof(cls) == size, name
        for f, _ in cls._fields_:
            assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert int(out["rt_path.reserved"]) == A.Path.reserved.offset == 44   # the tag: word 11, name and place kept


def test_path_symbols_resolve(rt):
    lib = rt.lib()
    assert len(NEW_SYMBOLS) == 12
    for name in NEW_SYMBOLS:
        assert name in rt._abi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name


def test_paths_tag_is_word_11(rt):
    p = rt.Renderer.make_paths(np.arange(3))
    p.buffer.view(np.uint32)[:, 11] = [7, 8, 0x80000001]
    assert p.tag.view(np.uint32).tolist() == [7, 8, 0x80000001]


# ---- 2. the camera hook against the existing references ------------------------------------------------
@pytest.mark.parametrize("s", [0, 1])
def test_camera_hook_equals_references(rt, orc, s):
    rnd = rt.random_offsets(SEED, W, H)
    o, d, idx = sh.sample_rays(rt, orc, W, H, SEED, s)
    want_rays = rt.Renderer.make_rays(o, d)
    want_paths = rt.Renderer.make_paths(idx)
    rays, paths = rt.debug_camera_paths_host(uniforms(rt), rnd, s)
    assert rays.shape == (W * H, 8) and len(paths) == W * H
    assert same(rays, want_rays)
    assert np.array_equal(paths.sample.view(np.uint32), idx.astype(np.uint32))   # the Halton indices
    assert np.array_equal(paths.tag, np.arange(W * H))                            # stride 1, offset 0
    got = paths.buffer.copy()
    got.view(np.uint32)[:, 11] = 0   # make_paths knows no tag
    assert same(got, want_paths.buffer)
    assert np.all(rays[:, 3] == 0) and np.all(np.isinf(rays[:, 7]))


def test_camera_hook_frame_offset_and_extra_samples(rt):
    rnd = rt.random_offsets(SEED, W, H)
    u = uniforms(rt, frame=3, spp=2)
    u.enableMotionAdaptiveSampling, u.motionSamplingMaxExtraSamples = 1, 3
    for s in (0, 1):
        _, paths = rt.debug_camera_paths_host(u, rnd, s)
        want = (rnd.astype(np.uint64) + 3 * (2 + 3) + s).astype(np.uint32)
        assert np.array_equal(paths.sample.view(np.uint32), want)
    u.enableMotionAdaptiveSampling = 0   # maxExtra counts only while the feature is on
    _, paths = rt.debug_camera_paths_host(u, rnd, 1)
    assert np.array_equal(paths.sample.view(np.uint32), (rnd.astype(np.uint64) + 3 * 2 + 1).astype(np.uint32))
    # uint32 arithmetic: an offset near 2^32 wraps
    big = rnd.copy()
    big[:] = 0xFFFFFFFE
    _, paths = rt.debug_camera_paths_host(u, big, 1)
    assert np.all(paths.sample.view(np.uint32) == np.uint32((0xFFFFFFFE + 7) & 0xFFFFFFFF))


def test_camera_hook_subrange_and_tags(rt):
    rnd = rt.random_offsets(SEED, W, H)
    u = uniforms(rt)
    full_r, full_p = rt.debug_camera_paths_host(u, rnd, 1, tag_stride=4, tag_offset=3)
    assert np.array_equal(full_p.tag, np.arange(W * H) * 4 + 3)
    sub_r, sub_p = rt.debug_camera_paths_host(u, rnd, 1, first_pixel=9, n=11, tag_stride=4, tag_offset=3)
    assert sub_r.shape == (11, 8)
    assert same(sub_r, full_r[9:20]) and same(sub_p.buffer, full_p.buffer[9:20])
    _, one = rt.debug_camera_paths_host(u, rnd, 0)
    assert np.array_equal(one.tag, np.arange(W * H))


# ---- 3. errors without a device ------------------------------------------------------------------------
def test_null_ctx_is_rejected_by_every_entry_point(rt):
    L, A = rt.lib(), rt._abi
    E = A.RT_ERR_INVALID_ARG
    u, o = uniforms(rt), A.CameraOpts()
    o.tag_stride = 1
    buf = (C.c_float * 64)()
    st = (A.CompactStream * 1)()
    assert L.rt_camera_paths(None, C.byref(u), C.byref(o), buf, 1, buf, buf) == E
    assert L.rt_camera_paths_on(None, C.byref(u), C.byref(o), buf, 1, buf, buf, None) == E
    assert L.rt_compact_paths(None, buf, 1, 1, st, 0, buf, buf) == E
    assert L.rt_compact_paths_on(None, buf, 1, 1, st, 0, buf, buf, None) == E
    assert L.rt_connect_paths(None, buf, 1, buf, None, buf, 1) == E
    assert L.rt_connect_paths_on(None, buf, 1, buf, None, buf, 1, None) == E
    assert L.rt_retire_paths(None, buf, 1, buf, 1) == E
    assert L.rt_retire_paths_on(None, buf, 1, buf, 1, None) == E
    assert L.rt_average_samples(None, buf, 1, 1, buf) == E
    assert L.rt_average_samples_on(None, buf, 1, 1, buf, None) == E
    assert L.rt_last_error(None)   # message set, no crash


def test_camera_hook_rejects_bad_arguments(rt):
    L, A = rt.lib(), rt._abi
    E = A.RT_ERR_INVALID_ARG
    rnd = rt.random_offsets(SEED, W, H)
    u = uniforms(rt)
    rays, paths = np.empty((W * H + 1, 8), F), np.empty((W * H + 1, 12), F)
    assert rays.ctypes.data % 16 == 0 and paths.ctypes.data % 16 == 0

    def call(n=W * H, first=0, sample=0, stride=1, r=rays.ctypes.data, p=paths.ctypes.data, rn=rnd.ctypes.data, un=u):
        o = A.CameraOpts()
        o.first_pixel, o.sample, o.tag_stride = first, sample, stride
        return L.rt_debug_camera_paths_host(C.byref(un) if un is not None else None, C.byref(o), rn, n, r, p)

    assert call() == A.RT_OK
    assert call(n=W * H + 1) == E and call(first=30, n=6) == E and call(first=W * H, n=1) == E   # past the image
    assert call(first=W * H, n=0) == A.RT_OK and call(first=30, n=5) == A.RT_OK
    assert call(first=0xFFFFFFFF, n=2) == E                                                        # no 32-bit wrap
    assert call(sample=-1) == E
    assert call(stride=0) == E
    assert call(r=rays.ctypes.data + 8) == E and call(p=paths.ctypes.data + 4) == E and call(rn=rnd.ctypes.data + 2) == E
    assert call(n=W * H - 1, r=rays.ctypes.data + 32, p=paths.ctypes.data + 48) == A.RT_OK       # 16-byte aligned is enough
    assert call(r=None) == E and call(p=None) == E and call(rn=None) == E and call(un=None) == E
    bad = uniforms(rt)
    bad.width = 0
    assert call(un=bad) == E
    with pytest.raises(rt.RTError):
        rt.debug_camera_paths_host(u, rnd, 0, first_pixel=30, n=6)


def test_compact_hook_equals_numpy_and_checks_arguments(rt):
    """rt_debug_compact_paths_host: the sequential statement of rt_compact_paths and its argument
    checks, which the device entry point shares."""
    L, A = rt.lib(), rt._abi
    E = A.RT_ERR_INVALID_ARG
    rng = np.random.default_rng(3)
    n = 300
    paths = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint32)
    paths[:, 7] = rng.integers(0, 4, n)
    srcs = [rng.integers(0, 2 ** 32, (n, 4 * w), dtype=np.uint32) for w in (1, 2, 3, 4)]
    dsts = [np.full_like(x, 0xDEADBEEF) for x in srcs]
    index, count = np.full(n, 0xDEADBEEF, np.uint32), np.zeros(1, np.uint32)

    def streams(pairs):
        arr = (A.CompactStream * max(len(pairs), 1))()
        for k, (s, d, w) in enumerate(pairs):
            arr[k].src, arr[k].dst, arr[k].words = s, d, w
        return arr

    good = [(s.ctypes.data, d.ctypes.data, s.shape[1] // 4) for s, d in zip(srcs, dsts)]

    def call(pairs=good, mask=1, cnt=None, idx=index.ctypes.data, p=paths.ctypes.data, k=None):
        return L.rt_debug_compact_paths_host(p, n, mask, streams(pairs), len(pairs) if k is None else k, idx,
                                             count.ctypes.data if cnt is None else cnt)

    for mask in (1, 2, 3):
        for d in dsts:
            d[:] = 0xDEADBEEF
        index[:] = 0xDEADBEEF
        assert call(mask=mask) == A.RT_OK
        sel = (paths[:, 7] & mask) != 0
        m = int(sel.sum())
        assert count[0] == m and 0 < m < n
        assert np.array_equal(index[:m], np.nonzero(sel)[0]) and np.all(index[m:] == 0xDEADBEEF)
        for s, d in zip(srcs, dsts):
            assert np.array_equal(d[:m], s[sel]) and np.all(d[m:] == 0xDEADBEEF)
    assert call(idx=None) == A.RT_OK and call(pairs=[]) == A.RT_OK
    assert call(mask=0) == E
    assert call(pairs=good + [good[0]], k=5) == E
    assert call(pairs=[(good[0][0], good[0][1], 5)]) == E and call(pairs=[(good[0][0], good[0][1], 0)]) == E
    assert call(pairs=[(good[0][0], good[0][0], 1)]) == E                        # in place
    assert call(pairs=[good[0], (good[1][0], good[0][1], 2)]) == E               # two streams, one dst
    assert call(pairs=[(good[2][0], paths.ctypes.data, 3)]) == E                 # dst is paths
    assert call(pairs=[(paths.ctypes.data, good[2][1], 3)]) == A.RT_OK           # paths may be a src
    assert call(idx=index.ctypes.data + 2) == E and call(cnt=count.ctypes.data + 1) == E
    assert call(pairs=[(good[0][0] + 8, good[0][1], 1)]) == E
    assert call(p=None) == E and call(cnt=0) == E
