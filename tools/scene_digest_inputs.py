"""Inputs of tools/scene_digest.cpp beyond the presets: the seeds of tools/fuzz_seeds.py (the skinned,
animated, textured asset in each encoding), composed scenes from the fixtures of
tests/test_usd_compose.py (sublayer + override, reference, variant, reference inside a package) and
the inputs of the error paths.  Usage: python tools/scene_digest_inputs.py DIR"""
import copy
import os
import subprocess
import sys

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(R, "tests"))
import usd_writers as W  # noqa: E402
from test_usd import TEX, robot_prims  # noqa: E402
from test_usd_compose import HEAD, BOX  # noqa: E402

d = sys.argv[1]
subprocess.run([sys.executable, os.path.join(R, "tools", "fuzz_seeds.py"), d], check=True, stdout=subprocess.DEVNULL)
prims, _ = robot_prims()
os.makedirs(os.path.join(d, "textures"), exist_ok=True)
files = {
    "robot.usda": W.write_usda(prims),
    "robot.usdc": W.write_usdc(prims),
    "textures/tex.png": TEX,
    "sub_over.usda": (HEAD % "    subLayers = [@./robot.usda@]\n" +
                      'over "Robot"\n{\n    over "Looks"\n    {\n        over "Red"\n        {\n            over "PBR"\n'
                      '            {\n                color3f inputs:diffuseColor = (0.25, 0.5, 0.75)\n            }\n'
                      '        }\n    }\n}\n').encode(),
    "ref_root.usda": (HEAD % '    defaultPrim = "World"\n' + 'def Xform "World"\n{\n    def SkelRoot "Robot" (\n'
                      '        prepend references = @./robot.usdc@</Robot>\n    )\n    {\n    }\n}\n').encode(),
    "var_full.usda": (HEAD % "" + (
        'def Xform "World" (\n%s    prepend variantSets = "lod"\n)\n{\n    variantSet "lod" = {\n'
        '        "full" {\n            def SkelRoot "Robot" (\n                references = @./robot.usda@</Robot>\n'
        '            )\n            {\n            }\n        }\n        "proxy" {\n%s        }\n    }\n}\n') % (
        '    variants = {\n        string lod = "full"\n    }\n', BOX)).encode(),
    "composed.usdz": W.write_usdz(
        "scene.usda", (HEAD % '    defaultPrim = "World"\n' + 'def Xform "World"\n{\n    def SkelRoot "Robot" (\n'
                       '        references = @./robot.usdc@</Robot>\n    )\n    {\n    }\n}\n').encode(),
        [("robot.usdc", W.write_usdc(prims)), ("textures/tex.png", TEX)]),
    # error paths
    "truncated.usdc": W.write_usdc(prims)[:-40],
    "nolayer.usdz": W.write_usdz("readme.txt", b"no layer here", [("textures/tex.png", TEX)]),
}
bad = copy.deepcopy(prims)
for a in bad[3]["attrs"]:
    if a["name"] == "primvars:skel:jointIndices":
        a["value"] = [7] + list(a["value"][1:])
files["badjoint.usda"] = W.write_usda(bad)
for k, v in files.items():
    with open(os.path.join(d, k), "wb") as f:
        f.write(v)
