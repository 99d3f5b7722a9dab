"""The host-checkable facts behind the frame kernels' shadow-ray skip, through
tools/shadow_skip_check.cpp, a stand-alone host program compiled from the kernels' own header
(csrc/rt_scatter.h):

* a shadow ray whose contribution is ±0 in every component (shadow_is_dark) cannot change the
  accumulator: a + c has the bits of a for every a that is not -0, so the ray need not be traced;
  shadow_is_dark is false as soon as one component is a NaN, a denormal or any other non-zero;
* what load_tabs stages for a spotlight (spot_cone) and what the query policy computes on the spot
  are cos_pinned(coneAngle) / normalize(direction) of the record bit for bit, for the presets'
  lights and 1,000 random records.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the compiler build() uses


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shadow_skip") / "shadow_skip_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                    os.path.join(ROOT, "tools", "shadow_skip_check.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def test_zero_contribution_leaves_the_accumulator(check):
    r = subprocess.run([check, "add", "1000000", "20240917"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1000000 accumulators x 8 zero vectors, 1000000 non-zero vectors, 0 failures" in r.stdout


def _random_lights(rt, n, seed):
    """Records of every type with directions from denormal to huge lengths (and exact axes) and cone
    angles over [0, pi] and a little beyond."""
    A = rt._abi
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = A.Light()
        L.type = int(rng.integers(0, 4)) if k % 4 else A.LightTypeSpotlight
        scale = np.float32(10.0) ** np.float32(rng.uniform(-20.0, 18.0))
        d = (rng.standard_normal(3).astype(np.float32) * scale).astype(np.float32)
        if k % 7 == 0:
            d[int(rng.integers(0, 3))] = 0.0
        L.direction = A.Float3(float(d[0]), float(d[1]), float(d[2]), 0.0)
        L.coneAngle = float(np.float32(rng.uniform(-0.1, 3.3)))
        L.position = A.Float3(*[float(x) for x in rng.standard_normal(3)], 0.0)
        L.color = A.Float3(4.0, 4.0, 4.0, 0.0)
        out.append(L)
    return out


def test_staged_spotlight_values(rt, assets, check, tmp_path):
    A = rt._abi
    assert C.sizeof(A.Light) == 128
    recs = []
    for name in ("c1", "c2", "c3g", "c3r"):
        d = rt.Scene.preset(name, assets).desc()
        recs.append(C.string_at(d.lights, int(d.light_count) * 128))
    n_preset = sum(len(r) for r in recs) // 128
    assert n_preset >= 4
    recs += [bytes(L) for L in _random_lights(rt, 1000, 5)]
    path = tmp_path / "lights.bin"
    path.write_bytes(b"".join(recs))
    r = subprocess.run([check, "spot", str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"spot: {n_preset + 1000} records" in r.stdout and "0 failures" in r.stdout
