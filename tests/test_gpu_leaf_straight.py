"""The leaf pass of the rotated kernels with the scene in LDS in one straight run (wurblpt_amd/csrc/wpt_triangle.h,
triangleTestRotatedStraight; wpt_pathtrace_body.inc.h): every lane of a pass computes det, T, the range condition, 1 / det and a,
and a rejected lane's values are thrown away in selects, where the parent skipped them in exec-mask regions.

1. The self test's form 4 (rayAuxRotated + the straight form with the walk's arguments) over the seven sets of
   tests/triangle_rotated.cpp and the set of tests/triangle_straight.cpp, 2^18 cases each: every word is the host's, as
   tests/test_gpu_triangle.py holds forms 0 - 3.  (The light-pdf loop keeps triangleTestRotated: its straight form lost its A/B,
   profiles/leaf_straight_cornell.txt, so there is no form 5.)
2. Frames, bit for bit the oracle's, of scenes that each make one formerly skipped region matter while other lanes of the wave
   take the other side: the Cornell box as it is; the box scaled by 2^-34 (every test enters the double-precision fall-back); the
   box with a zero-area triangle in its interior (two corners of a triangle of the short box coincide: V = 0 and W = -U exactly, so
   det == 0 and 1 / det is infinite in every lane that tests it, beside lanes that accept a wall); the box with min_hit_distance at
   a tenth of its size (the range test rejects near hits).  Each at 64 x 64 pixels -- four workgroups of 1024 lanes -- in the
   plain large kernel.  The sliced twin is launched for pooled frames only, which have more pixels than the device has lanes in
   flight (tests/test_gpu_sliced.py), so it renders 640 x 512 pixels at 4 spp: a band of eight rows across the boxes against the
   oracle, and the whole frame against the launch with one lane per pixel (the plain kernel).
3. One scene under WPT_WALK_SMALL_WORKGROUPS, unpooled and pooled: the small rotated units run the same leaf pass."""
import numpy as np
import pytest

from tests import scene_scale
from tests import triangle_cases as tc
from tests import triangle_straight_cases as stc
from tests.test_gpu_ordered_boxes import LARGE, ROTATED, SMALL, bits_differing, ran
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

N = 1 << 18
FORMS = {4: "rayAuxRotated + triangleTestRotatedStraight"}
SCENES = {"plain box": 4, "fall-back": 3, "degenerate triangle": 3, "large min_hit_distance": 2}     # samples_sqrt
POOLED = (640, 512)       # 327 680 pixels against 262 144 lanes in flight on an MI355X
BAND = (250, 8)           # eight rows across the boxes


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


# ---- 1. the self test ----

@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the host data, checked before any GPU work"""
    s, report, kinds, out = stc.run(tmp_path_factory.mktemp("leaf_straight_cases"), N)
    assert "total: 0 differences" in out and kinds is not None, out
    tc.check_shares({name: s[name] for name in tc.SETS})
    return s


@pytest.fixture(scope="module")
def device_words(dev, sets):
    """{(set, form): uint32 [N, 8]}, every launch made once"""
    return {(name, form): dev.selftest_triangle(form, w[:, :17].view(np.float32)) for name, w in sets.items() for form in FORMS}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", stc.SETS)
def test_device_words_are_the_hosts(sets, device_words, name, form):
    host_words, got = sets[name], device_words[(name, form)]
    want = host_words[:, tc.ACCEPTED:tc.W + 1]
    have = got[:, 0:6]
    both_nan = tc.is_nan(want) & tc.is_nan(have)
    bad = (want != have) & ~both_nan
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, "%s, %s: %d of %d cases differ (in words %s), the first: case %d, host %s, device %s" % (
        name, FORMS[form], rows.size, len(host_words), np.nonzero(bad.any(axis=0))[0].tolist(), rows[0],
        ["%08x" % x for x in want[rows[0]]], ["%08x" % x for x in have[rows[0]]])
    assert np.array_equal(got[:, 6], host_words[:, tc.K_ROTATED]), (name, FORMS[form], "RayAux::k")
    assert not got[:, 7].any()


# ---- 2. frames ----

def interior_triangle(sc):
    """the triangle that is no light's and whose centroid lies nearest the middle of the scene"""
    d = sc.d
    root = d.nodes[0]
    mid = 0.5 * (np.array(root.lo[:], np.float64) + np.array(root.hi[:], np.float64))
    g = scene_scale._floats(d.tri_geom, d.tri_count, _abi.TriGeom)
    lights = {int(d.hotspots[i].prim) for i in range(int(d.hotspot_count))}
    centroid = (g[:, 0:3].astype(np.float64) + g[:, 4:7] + g[:, 8:11]) / 3.0
    order = np.argsort(((centroid - mid) ** 2).sum(axis=1))
    return int(next(t for t in order if int(t) not in lights))


def make(name, width, height):
    """(scene, parameters) of one of SCENES at a frame size"""
    sc = host.cornell(width, height, 1, 2)
    p = host.default_params()
    if name == "fall-back":
        scene_scale.scale_scene(sc, -34)
        p = scene_scale.scaled_params(-34)
    elif name == "degenerate triangle":
        g = scene_scale._floats(sc.d.tri_geom, sc.d.tri_count, _abi.TriGeom)
        t = interior_triangle(sc)
        g[t, 8:11] = g[t, 0:3]            # the third corner on the first: the tree's boxes still hold the triangle
    elif name == "large min_hit_distance":
        root = sc.d.nodes[0]
        p.min_hit_distance = float(np.float32(0.1 * max(hi - lo for lo, hi in zip(root.lo[:], root.hi[:]))))
    return sc, p


def reference(oracle, name, sc, s, p, block=None):
    """the oracle's frame, after the guards: finite, not black; for the scaled box nearly every test in the fall-back; the
    degenerate triangle is tested often (V = 0 takes every test of it, and hardly any other, into the fall-back)"""
    oracle.triangle_tally()
    ref, _ = oracle.render(sc, s, params=p, block=block)
    tests, fallback = oracle.triangle_tally()
    share = {"fall-back": (0.99, 1.0), "degenerate triangle": (0.002, 0.05)}.get(name, (0.0, 0.001))
    assert tests > 1000 and share[0] * tests <= fallback <= share[1] * tests, (name, tests, fallback)
    rendered = ref if block is None else ref.reshape(-1, 3)[block[0]:block[0] + block[1]]
    assert np.isfinite(ref).all() and rendered.mean() > 0.001, (name, float(rendered.mean()))
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def small_frames(oracle):
    """{scene: (scene, parameters, samples_sqrt, the oracle's 64 x 64 frame)}, made once; the changed scenes do change the frame"""
    out = {}
    for name, s in SCENES.items():
        sc, p = make(name, 64, 64)
        out[name] = (sc, p, s, reference(oracle, name, sc, s, p))
    plain = host.cornell(64, 64, 1, 2)
    for name in ("degenerate triangle", "large min_hit_distance"):
        assert bits_differing(out[name][3], oracle.render(plain, out[name][2])[0]) > 0, name
    return out


def render(dev, sc, s, p, walk=0, slices=0, variant=0):
    """(frame, what ran) of one launch"""
    ds = dev.DeviceScene(sc)
    try:
        dev.lib().wpt_set_walk(walk)
        dev.lib().wpt_set_launch_config(0, variant)
        dev.set_slices(slices)
        got, _ = ds.render(s, params=p)
        return got, ran(dev)
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_launch_config(0, 0)
        dev.lib().wpt_set_walk(0)
        ds.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_plain_large_kernel_renders_the_oracles_frame(dev, small_frames, name):
    sc, p, s, ref = small_frames[name]
    got, what = render(dev, sc, s, p)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert bits_differing(got, ref) == 0, (name, bits_differing(got, ref))


def pooled(dev, oracle, name, walk, workgroup):
    """the sliced twin on a pooled frame: a band against the oracle, the whole frame against the launch with one lane per pixel"""
    sc, p = make(name, *POOLED)
    w = POOLED[0]
    ref = reference(oracle, name, sc, 2, p, block=(BAND[0] * w, BAND[1] * w))
    band = slice(BAND[0], BAND[0] + BAND[1])
    got, what = render(dev, sc, 2, p, walk=walk, slices=2)
    assert what == ("wpt_pathtrace", ROTATED + ", sliced x2", workgroup), what
    one_lane_per_pixel, what = render(dev, sc, 2, p, walk=walk, variant=0x10)
    assert what == ("wpt_pathtrace", ROTATED, workgroup), what
    assert bits_differing(got[band], ref[band]) == 0, (name, bits_differing(got[band], ref[band]))
    assert bits_differing(got, one_lane_per_pixel) == 0, (name, bits_differing(got, one_lane_per_pixel))


@pytest.mark.parametrize("name", list(SCENES))
def test_sliced_twin_renders_the_oracles_rows(dev, oracle, name):
    pooled(dev, oracle, name, 0, LARGE)


# ---- 3. the small form ----

def test_small_workgroups(dev, oracle, small_frames):
    name = "degenerate triangle"
    sc, p, s, ref = small_frames[name]
    got, what = render(dev, sc, s, p, walk=dev.WALK_SMALL_WORKGROUPS)
    assert what == ("wpt_pathtrace", ROTATED, SMALL), what
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)
    pooled(dev, oracle, name, dev.WALK_SMALL_WORKGROUPS, SMALL)
