"""C-ABI boundary of the device ray queries (rt_trace_closest / rt_trace_any / rt_get_query_stats)
on CPU: the record layouts the header declares equal the ctypes mirrors, and the entry points
answer NULL arguments with a status."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT


def test_query_struct_layouts_match_c(rt, tmp_path):
    A = rt._abi
    stats_fields = [n for n, _ in A.QueryStats._fields_]
    hit_fields = [n for n, _ in A.RayHit._fields_]
    ray_fields = [n for n, _ in A.Ray._fields_]
    lines = ["P(rt_ray); P(rt_ray_hit); P(rt_query_stats);"]
    lines += [f"O(rt_ray, {f});" for f in ray_fields]
    lines += [f"O(rt_ray_hit, {f});" for f in hit_fields]
    lines += [f"O(rt_query_stats, {f});" for f in stats_fields]
    prog = tmp_path / "qlayout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  ''' + "\n  ".join(lines) + r'''
  printf("RT_MISS %u\n", RT_MISS);
  return 0;
}''')
    exe = tmp_path / "qlayout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["rt_ray"]) == C.sizeof(A.Ray) == 32
    assert int(out["rt_ray_hit"]) == C.sizeof(A.RayHit) == 32
    assert int(out["rt_query_stats"]) == C.sizeof(A.QueryStats)
    for name, cls, fields in (("rt_ray", A.Ray, ray_fields), ("rt_ray_hit", A.RayHit, hit_fields),
                              ("rt_query_stats", A.QueryStats, stats_fields)):
        for f in fields:
            assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    # the two 16-B words of each record
    assert A.Ray.direction.offset == 16 and A.Ray.tmax.offset == 28
    assert A.RayHit.triangle.offset == 12 and A.RayHit.mesh.offset == 16 and A.RayHit.reserved.offset == 28
    assert int(out["RT_MISS"]) == A.RT_MISS == 0xFFFFFFFF
    # rt_stats keeps its layout: the query figures live in their own struct
    assert not any(n.startswith("query") for n, _ in A.Stats._fields_)


def test_query_null_arguments_return_status(rt):
    lib = rt.lib()
    E = rt._abi.RT_ERR_INVALID_ARG
    buf = (C.c_float * 8)()
    assert lib.rt_trace_closest(None, None, 0, None) == E
    assert lib.rt_trace_closest(None, buf, 1, buf) == E
    assert lib.rt_trace_any(None, None, 1, None) == E
    assert lib.rt_trace_closest_on(None, None, 1, None, None) == E
    assert lib.rt_trace_any_on(None, buf, 1, buf, None) == E
    assert lib.rt_get_query_stats(None, None) == E
    qs = rt._abi.QueryStats()
    assert lib.rt_get_query_stats(None, C.byref(qs)) == E
    assert lib.rt_last_error(None)   # message set, no crash


def test_on_twins_and_query_module(rt):
    """Every `_on` entry point is its plain form plus a trailing stream handle, and the package's
    query names are the queries submodule's."""
    import importlib
    lib, A = rt.lib(), rt._abi
    assert len(A.ON_TWINS) == len(set(A.ON_TWINS)) == 11
    for name in A.ON_TWINS:
        plain, on = getattr(lib, name), getattr(lib, name + "_on")
        assert on.argtypes == plain.argtypes + [C.c_void_p], name
        assert on.restype == plain.restype, name
        assert name in A.EXPORTED_SYMBOLS and name + "_on" in A.EXPORTED_SYMBOLS, name
    assert sorted(n[:-3] for n in A.EXPORTED_SYMBOLS if n.endswith("_on")) == sorted(A.ON_TWINS)
    Q = importlib.import_module(rt.__name__ + ".queries")
    for name in ("Hits", "Surface", "Paths", "Shaded", "Compacted", "debug_trace_host", "debug_resolve_host",
                 "debug_shade_host", "debug_camera_paths_host"):
        assert getattr(rt, name) is getattr(Q, name), name
    assert issubclass(rt.Renderer, Q.RendererQueries)
    for name in ("make_rays", "trace", "resolve", "make_paths", "shade", "camera_paths", "compact", "connect", "retire",
                 "average", "_path_buffers", "path_trace", "query_stats"):
        assert callable(getattr(rt.Renderer, name)) and name in vars(Q.RendererQueries), name


def test_make_rays_host_layout(rt):
    o = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    d = np.array([[0, 0, 1], [0, 2, 0]], np.float32)
    r = rt.Renderer.make_rays(o, d)
    assert r.dtype == np.float32 and r.shape == (2, 8) and r.flags.c_contiguous
    assert np.array_equal(r[:, 0:3], o) and np.array_equal(r[:, 4:7], d)
    assert np.all(r[:, 3] == 0) and np.all(np.isinf(r[:, 7]))
    r = rt.Renderer.make_rays(o, d, tmax=[0.5, 2.0])
    assert r[:, 7].tolist() == [0.5, 2.0]
    rec = np.frombuffer(r.tobytes(), dtype=np.dtype(rt._abi.Ray))   # the same bytes as rt_ray records
    assert rec["direction"][1].tolist() == [0, 2, 0] and rec["tmax"][0] == 0.5
