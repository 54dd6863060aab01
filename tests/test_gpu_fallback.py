"""Every kernel family through the double-precision fall-back of the watertight triangle test (wpt_triangle.h: |U|, |V| or |W|
below 2^-63).  The scenes we usually render almost never reach it (Cornell box 32x32, 9 spp: 0 of 306 020 triangle tests), so
these are the same scenes scaled by 2^-34 (tests/scene_scale.py): the same scene in exact arithmetic, and every triangle test
takes the fall-back.  Each render first asserts on the CPU, from the restatement's own tally, that at least 99 % of its triangle
tests entered the fall-back and that its frame is finite and not black; then the device's frame (and counters, where the launch
counts) must be the restatement's bit for bit.  At 2^-40 products of two coordinates' differences reach the denormal range: the
production kernels must still render the restatement's bits there.

Left out: scenes the scaling helper does not cover (a camera with lens distortion, an animated camera); measured-BRDF,
time-of-flight and animated scenes are not scaled here."""
import os

import numpy as np
import pytest

from tests import scene_scale
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

E = -34
OBJ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj", "scene.obj")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_differing(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def reference(oracle, sc, s, params, block=None, share=0.99):
    """the restatement's frame and counters, after the conditions that make the comparison one of the fall-back"""
    oracle.triangle_tally()
    ref, counters = oracle.render(sc, s, params=params, block=block)
    tests, fallback = oracle.triangle_tally()
    assert tests > 1000 and fallback >= share * tests, (tests, fallback)
    assert np.isfinite(ref).all() and ref.mean() > 0.01, ref.mean()
    ref.setflags(write=False)
    return ref, counters


class Scaled:
    """a scene scaled by 2^exponent, its parameters, its upload and the restatement's frame at s x s samples"""

    def __init__(self, dev, oracle, sc, s, exponent=E):
        self.sc, self.s = sc, s
        scene_scale.scale_scene(sc, exponent)
        self.p = scene_scale.scaled_params(exponent)
        self.ref, self.counters = reference(oracle, sc, s, self.p)
        self.ds = dev.DeviceScene(sc)


@pytest.fixture(scope="module")
def cornell(dev, oracle):
    return Scaled(dev, oracle, host.cornell(48, 40, 1, 2), 3)


def render(dev, c, walk=0, variant=0, with_counters=False):
    """(frame, counters, kernel name, kernel form) of one launch under wpt_set_walk(walk) and launch variant `variant`"""
    try:
        dev.lib().wpt_set_walk(walk)
        dev.lib().wpt_set_launch_config(0, variant)
        ds = c.ds if variant == 0 else dev.DeviceScene(c.sc)     # the variants of test_gpu_parity.py take their own upload
        got, counters = ds.render(c.s, params=c.p, with_counters=with_counters)
        return got, counters, dev.lib().wpt_kernel_name(), dev.lib().wpt_kernel_form()
    finally:
        dev.lib().wpt_set_walk(0)
        dev.lib().wpt_set_launch_config(0, 0)


LAUNCHES = {"default": (0, 0, b"rotated corners"), "select corners": (16, 0, b""), "no fold": (32, 0, b"rotated corners"),
            "variant 0x01": (0, 0x01, b""), "variant 0x02": (0, 0x02, b"")}


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_cornell_product_launch(dev, cornell, launch):
    walk, variant, form = LAUNCHES[launch]
    assert (walk, form) != (16, b"rotated corners") and dev.WALK_SELECT_CORNERS == 16 and dev.WALK_NO_FOLD == 32
    got, _, name, got_form = render(dev, cornell, walk, variant)
    assert name == b"wpt_pathtrace" and got_form == form, (name, got_form)
    if launch == "no fold":
        assert cornell.ds.folded_links() > 0                      # the default launch does fold in this scene's tree
    assert bits_differing(got, cornell.ref) == 0, (launch, bits_differing(got, cornell.ref))


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_cornell_counting_launch(dev, cornell, launch):
    walk, variant, _ = LAUNCHES[launch]
    got, counters, name, form = render(dev, cornell, walk, variant, with_counters=True)
    assert name == b"wpt_pathtrace" and form == b""                # counting launches keep the select form
    assert bits_differing(got, cornell.ref) == 0, (launch, bits_differing(got, cornell.ref))
    assert counters == cornell.counters, (launch, counters, cornell.counters)


def test_cornell_wavefront_form(dev, cornell):
    try:
        dev.lib().wpt_set_wavefront(1, 0, 0, 0)
        got, _ = cornell.ds.render(cornell.s, params=cornell.p)
        assert dev.lib().wpt_kernel_name() == b"wf_trace + wf_shade"
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert bits_differing(got, cornell.ref) == 0


def test_cornell_batch_of_two_views(dev, oracle, cornell):
    sc = cornell.sc
    f = np.float32(2.0) ** np.float32(E)
    root = sc.d.nodes[0]
    lo, hi = np.array(root.lo[:], np.float64), np.array(root.hi[:], np.float64)
    mid = 0.5 * (lo + hi) + 0.013 * (hi - lo)
    second = host.camera_looking_at(sc, mid, mid + np.array([float(f), 0.0, 0.3 * float(f)]))
    cams = [_abi.Camera.from_buffer_copy(sc.camera.contents), second]
    frames = cornell.ds.render_views(cornell.s, cams, params=cornell.p).cpu().numpy()
    assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace, views, scene in LDS"
    assert bits_differing(frames[0], cornell.ref) == 0
    saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
    try:
        sc.camera[0] = second
        ref, _ = reference(oracle, sc, cornell.s, cornell.p)
    finally:
        sc.camera[0] = saved
    assert bits_differing(ref, cornell.ref) > 0
    assert bits_differing(frames[1], ref) == 0


def test_cornell_adaptive_launch_with_a_mixed_map(dev, oracle, cornell):
    sc = cornell.sc
    m = np.array([0, 1, 2, 3])[np.random.default_rng(5).integers(0, 4, (sc.height, sc.width))].astype(np.uint16)
    frame = cornell.ds.render_adaptive(m, params=cornell.p).cpu().numpy()
    assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace, adaptive, scene in LDS"
    want = np.zeros_like(frame)
    for n in (1, 2, 3):
        ref = cornell.ref if n == cornell.s else reference(oracle, sc, n, cornell.p)[0]
        want[m == n] = ref[m == n]
    assert bits_differing(frame, want) == 0


def test_cornell_transient_launch_with_scaled_edges(dev, oracle, cornell):
    f = np.float32(2.0) ** np.float32(E)
    edges = dev.uniform_edges(0.0, 1.5, 8) * f                     # a power of two: the scaled edges are the edges of the scaled scene
    frame, bins = cornell.ds.render_transient(cornell.s, edges, params=cornell.p)
    assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace, transient, scene in LDS"
    assert bits_differing(frame, cornell.ref) == 0
    assert sum(int(bins[k].any()) for k in range(8)) >= 4
    lit = sorted(range(8), key=lambda k: -float(bins[k].sum()))[:2]      # the two bins that hold most of the light
    for k in lit:
        p = _abi.Params.from_buffer_copy(cornell.p)
        p.min_path_len = float(edges[k])
        p.max_path_len = float(np.nextafter(np.float32(edges[k + 1]), np.float32(-np.inf)))
        oracle.triangle_tally()
        ref, _ = oracle.render(cornell.sc, cornell.s, params=p)
        tests, fallback = oracle.triangle_tally()
        assert fallback >= 0.99 * tests > 0 and ref.any()
        assert bits_differing(bins[k], ref) == 0, k


def test_cornell_ground_truth(dev, oracle, cornell):
    oracle.triangle_tally()
    ref = oracle.ground_truth(cornell.sc, params=cornell.p)
    tests, fallback = oracle.triangle_tally()
    assert tests > 1000 and fallback >= 0.99 * tests, (tests, fallback)
    got = dev.ground_truth(cornell.ds, params=cornell.p)
    assert (ref["materials"] >= 0).mean() > 0.5
    for name in ref:
        same = (got[name].view(np.uint32) == ref[name].view(np.uint32)) | ((got[name] != got[name]) & (ref[name] != ref[name]))
        assert same.all(), (name, int((~same).sum()))


def test_cornell_pooled_frame_in_four_slices(dev, oracle):
    """640 x 512 at 16 spp: more pixels than the device holds lanes, so the pool hands them out, forced into four units"""
    sc = host.cornell(640, 512, 1, 2)
    scene_scale.scale_scene(sc, E)
    p = scene_scale.scaled_params(E)
    ref, _ = reference(oracle, sc, 4, p)
    ds = dev.DeviceScene(sc)
    try:
        dev.set_slices(4)
        got, _ = ds.render(4, params=p)
        form = dev.lib().wpt_kernel_form()
        taken, continued = dev.last_slice_stats()
    finally:
        dev.set_slices(0)
    ds.check()
    assert form == b"rotated corners, sliced x4" and taken + continued == 640 * 512 * 3, (form, taken, continued)
    assert bits_differing(got, ref) == 0
    try:
        dev.set_slices(4)
        dev.lib().wpt_set_walk(dev.WALK_SELECT_CORNERS)
        sel, _ = ds.render(4, params=p)
        assert dev.lib().wpt_kernel_form() == b", sliced x4"
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_walk(0)
    assert bits_differing(sel, ref) == 0


def test_random_triangles_plain_counting_and_wide(dev, oracle):
    plain = Scaled(dev, oracle, host.random_triangles(2000, 7, 56, 40), 3)
    got, _ = plain.ds.render(plain.s, params=plain.p)
    assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace"
    assert bits_differing(got, plain.ref) == 0
    counted, counters = plain.ds.render(plain.s, params=plain.p, with_counters=True)
    assert bits_differing(counted, plain.ref) == 0 and counters == plain.counters
    try:
        dev.lib().wpt_set_walk(dev.WALK_WIDE)                      # before the upload: the scene gets the wide form of its tree
        got, _ = dev.DeviceScene(plain.sc).render(plain.s, params=plain.p)
        assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace, wide walk"
    finally:
        dev.lib().wpt_set_walk(0)
    assert bits_differing(got, plain.ref) == 0


def test_obj_fixture_with_two_sided_materials(dev, oracle):
    f = float(np.float32(2.0) ** np.float32(E))
    sc = host.import_obj(OBJ, 40, 32, eye=(0.5 * f, 2.2 * f, 6.5 * f), at=(0.0, 1.2 * f, 0.0), import_bits=4, scale=f, env_radiance=0.05)
    assert sc is not None and sc.d.tri_count == 25
    p = scene_scale.scaled_params(E)
    ref, counters = reference(oracle, sc, 2, p)
    got, gc = dev.DeviceScene(sc).render(2, params=p, with_counters=True)
    assert bits_differing(got, ref) == 0 and gc == counters
    got, _ = dev.DeviceScene(sc).render(2, params=p)
    assert bits_differing(got, ref) == 0


@pytest.mark.parametrize("variant", [0, 0x02])
def test_cornell_in_the_denormal_range(dev, oracle, variant):
    """2^-40: the sheared coordinates are near 2^-40 and their products near 2^-80, the cross products of the light's pdf and the
    squares behind its distances reach below 2^-126.  The restatement's frame stays finite (its mean drops, 0.0257 against
    0.0436 at 32 x 32: light paths are lost to underflow, in the reference as well); the kernels must lose the same ones."""
    sc = host.cornell(48, 40, 1, 2)
    scene_scale.scale_scene(sc, -40)
    p = scene_scale.scaled_params(-40)
    oracle.triangle_tally()
    ref, _ = oracle.render(sc, 3, params=p)
    tests, fallback = oracle.triangle_tally()
    assert fallback == tests > 1000 and np.isfinite(ref).all() and ref.mean() > 0.01
    try:
        dev.lib().wpt_set_launch_config(0, variant)
        got, _ = dev.DeviceScene(sc).render(3, params=p)
        form = dev.lib().wpt_kernel_form()
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    assert form == (b"rotated corners" if variant == 0 else b"")
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)
