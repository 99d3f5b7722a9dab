"""Nothing throws across the rt_scene_* C-ABI: tools/scene_alloc_check.cpp makes the
N-th allocation of every entry point that can allocate fail, N = 0, 1, ... until the call succeeds,
as a stand-alone host program (tools/scene_alloc_check.sh; SANITIZE=1 there adds AddressSanitizer +
UBSan).  Every failing call must return RT_ERR_OUT_OF_MEMORY or RT_ERR_IO and leave a freeable
scene; an exception that escaped would end the program in std::terminate."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("add_obj", "add_usd", "add_procedural", "preset", "get_desc", "add_texture", "load_texture",
           "bind_texture", "joint_matrices", "set_lights")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_failed_allocations_return_a_status():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "scene_alloc_check.sh")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    for e in ENTRIES:
        assert f"rt_scene_{e} " in r.stdout and "first success" in r.stdout, r.stdout
    assert r.stdout.count("first success at N=") == len(ENTRIES), r.stdout
    # the readers do allocate: the campaign is not vacuous
    for e in ("add_obj", "add_usd", "add_procedural", "preset"):
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith(f"rt_scene_{e} "))
        assert int(line.split("N=")[1].split(";")[0]) > 10, line
