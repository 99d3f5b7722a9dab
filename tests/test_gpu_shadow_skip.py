"""Shadow rays the shading step resolves without a traversal: a ray whose
contribution is ±0 in every component is not traced by any frame kernel (shade_step,
rt_stats.dark_shadow_rays), and wf_shade adds the contribution of a ray its root word proves
unoccluded itself (rt_stats.root_unoccluded_shadow_rays).  Neither changes a bit of the frame or a
ray count: every variant -- bulk rounds (wf_shade shades every hit), the finish kernel from round 0,
bulk rounds then the finish kernel with team drain 4, bulk rounds with the hit sort, the megakernel
-- equals the CPU oracle in radiance, depth, motion and closest / shadow ray counts, on frames the
oracle gives 230 / 8,222, 319 / 5,298 and 726 / 6,673 dark / all shadow rays."""
import numpy as np
import pytest

from helpers import parity_report

pytestmark = pytest.mark.gpu

#        preset  W   H  spp bounces seed
CASES = {"c1_64x64": ("c1", 64, 64, 2, 4, 1), "c1_96x64": ("c1", 96, 64, 1, 2, 3), "c2_64x48": ("c2", 64, 48, 2, 4, 1)}
# dark / all shadow rays of each case's first frame, counted at the oracle's shadow-ray site (contribution == 0)
ORACLE_DARK = {"c1_64x64": (230, 8222), "c1_96x64": (319, 5298), "c2_64x48": (726, 6673)}
# Renderer arguments; whether wf_shade runs (bulk rounds: tail_paths=1 is "no finish kernel")
VARIANTS = {
    "bulk": (dict(pipeline="wavefront", tail_paths=1), True),
    "finish": (dict(pipeline="wavefront", tail_paths=1 << 30), False),
    "team4": (dict(pipeline="wavefront", tail_paths=1024, tuning={"team": 4}), True),
    "sort": (dict(pipeline="wavefront", tail_paths=1, sort_bins=1024), True),
    "megakernel": (dict(pipeline="megakernel"), False),
}


def _renderer(rt, scenes, case, **kw):
    preset, W, H, spp, bounces, seed = CASES[case]
    R = rt.Renderer(scenes[preset], W, H, seed=seed, **kw)
    R.samplesPerPixel, R.maxBounces = spp, bounces
    return R


def _frame(R):
    R.wait()
    depth, motion, _ = R.aux()
    return R.radiance(), depth, motion, R.stats()


@pytest.fixture(scope="module")
def scenes(rt, assets):
    return {p: rt.Scene.preset(p, assets) for p in ("c1", "c2")}


@pytest.fixture(scope="module")
def ref(rt, orc, scenes):
    """Per case the oracle's first two frames (every renderer of a case draws the same uniforms), and
    the megakernel's dark-ray count of the first: the per-path arithmetic is one, so every variant
    must count the same rays."""
    out = {}
    for case, (preset, *_rest) in CASES.items():
        R = _renderer(rt, scenes, case, pipeline="megakernel")
        us = [R.draw()]
        R.wait()
        dark = int(R.stats().dark_shadow_rays)
        us.append(R.draw())
        R.wait()
        rnd = R.random
        R.close()
        osc = orc.OracleScene(scenes[preset].desc())
        frames, prev, motion = [], None, None
        for u in us:
            o = osc.render(u, rnd, accum_in=prev, motion_in=motion)
            prev, motion = o["radiance"], o["motion"]
            frames.append(o)
        assert (dark, frames[0]["shadow_rays"]) == ORACLE_DARK[case], case
        out[case] = (frames, dark)
    return out


def _assert_oracle(got, o, what):
    g, depth, motion, st = got
    rep = parity_report(g, o["radiance"])
    print(what, rep, "closest", st.closest_rays, "shadow", st.shadow_rays, "dark", st.dark_shadow_rays, "root-unoccluded",
          st.root_unoccluded_shadow_rays, "trace", st.trace_rays)
    assert rep["n_bad"] == 0, (what, rep)
    assert np.array_equal(depth, o["depth"]) and np.array_equal(motion, o["motion"]), what
    assert st.closest_rays == o["closest_rays"] and st.shadow_rays == o["shadow_rays"], what
    assert st.paths == o["paths"], what


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_and_counts_equal_the_oracle(rt, scenes, ref, case, variant):
    kw, shades = VARIANTS[variant]
    frames, dark = ref[case]
    R = _renderer(rt, scenes, case, **kw)
    R.draw()
    got = _frame(R)
    R.close()
    st = got[3]
    _assert_oracle(got, frames[0], (case, variant))
    assert st.dark_shadow_rays > 0
    assert st.dark_shadow_rays == dark            # the same rays in every kernel that shades
    assert st.total_dark_shadow_rays == st.dark_shadow_rays
    if shades:
        assert st.root_unoccluded_shadow_rays > 0
        assert st.total_root_unoccluded_shadow_rays == st.root_unoccluded_shadow_rays
    else:
        assert st.root_unoccluded_shadow_rays == 0   # the finish kernel and the megakernel have no root word
    assert st.dark_shadow_rays <= st.shadow_rays and st.root_unoccluded_shadow_rays <= st.shadow_rays
    assert st.dark_shadow_rays + st.root_unoccluded_shadow_rays <= st.shadow_rays   # a ray is in one class
    if variant in ("bulk", "sort"):   # no finish kernel: every ray is wf_trace's or resolved by a producer
        assert st.trace_rays == st.closest_rays + st.shadow_rays


@pytest.mark.parametrize("variant", ["bulk", "finish", "megakernel"])
def test_counting_frame(rt, scenes, ref, variant):
    """The counting kernels: the same frame and ray counts; a skipped ray adds no visit, the others do."""
    case = "c1_64x64"
    R = _renderer(rt, scenes, case, **VARIANTS[variant][0])
    R.set_counting(True)
    R.draw()
    got = _frame(R)
    R.close()
    st = got[3]
    _assert_oracle(got, ref[case][0][0], (case, variant, "counting"))
    assert st.node_visits > 0 and st.tri_tests > 0
    assert st.dark_shadow_rays == ref[case][1]
    if variant == "bulk":
        assert st.trace_rays == st.closest_rays + st.shadow_rays
        assert st.trace_nodes == st.node_visits and st.trace_tris == st.tri_tests


@pytest.mark.parametrize("variant", ["bulk", "team4"])
def test_two_frames_in_flight(rt, scenes, ref, variant):
    """Two frames submitted back to back on two slots: the second equals the one a renderer with one
    frame in flight produces, bit for bit, and both equal the oracle's second frame."""
    case = "c1_64x64"
    kw = VARIANTS[variant][0]
    got = []
    for fif in (1, 2):
        R = _renderer(rt, scenes, case, frames_in_flight=fif, **kw)
        R.draw()
        if fif == 1:
            R.wait()
        R.draw()
        got.append(_frame(R))
        assert R.stats().frames_in_flight == fif
        R.close()
    one, two = got
    for a, b in zip(one[:3], two[:3]):
        assert np.array_equal(a, b)
    for k in ("closest_rays", "shadow_rays", "dark_shadow_rays", "root_unoccluded_shadow_rays"):
        assert getattr(one[3], k) == getattr(two[3], k), k
    _assert_oracle(two, ref[case][0][1], (case, variant, "second frame, two in flight"))
    assert two[3].dark_shadow_rays > 0 and two[3].root_unoccluded_shadow_rays > 0
