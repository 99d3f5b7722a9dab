"""Device-count queries at the C-ABI boundary, on the CPU: the fourteen _indirect entry points
are declared in include/rt_api.h, exported by the library and listed in _abi.EXPORTED_SYMBOLS,
rt_device_count has the layout the ctypes mirror gives it, and a NULL context is an error status,
not a crash."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

QUERIES = ("rt_trace_closest", "rt_trace_any", "rt_resolve_hits", "rt_shade_hits", "rt_compact_paths", "rt_connect_paths",
           "rt_retire_paths")
SYMBOLS = [q + on + "_indirect" for q in QUERIES for on in ("", "_on")]   # of the plain and of the _on entry point


def test_fourteen_symbols_declared_exported_and_listed(rt):
    src = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", src))
    lib = rt.lib()
    assert len(SYMBOLS) == 14
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in rt._abi.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and C.POINTER(rt._abi.DeviceCount) in fn.argtypes, name
    # no indirect form of the two queries whose sizes the host knows
    assert not any(s.startswith(("rt_camera_paths_indirect", "rt_average_samples_indirect")) for s in declared)


def test_device_count_layout_matches_c(rt, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(rt_device_count), offsetof(rt_device_count, count), offsetof(rt_device_count, max),
         offsetof(rt_device_count, _pad));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    size, o_count, o_max, o_pad = map(int, subprocess.check_output([str(exe)]).split())
    D = rt._abi.DeviceCount
    assert size == 16 == C.sizeof(D)
    assert (o_count, o_max, o_pad) == (D.count.offset, D.max.offset, D._pad.offset) == (0, 8, 12)


def test_null_context_returns_status(rt):
    lib, A = rt.lib(), rt._abi
    cnt = A.DeviceCount()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        args = [C.byref(cnt) if t == C.POINTER(A.DeviceCount) else (0 if t is C.c_uint32 else None) for t in fn.argtypes]
        assert fn(*args) == A.RT_ERR_INVALID_ARG, name
    assert lib.rt_last_error(None)
