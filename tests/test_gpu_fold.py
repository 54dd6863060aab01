"""The kernels with the scene in LDS fold first children that repeat their parent's box out of their copy of the tree
(wurblpt_amd/csrc/wpt_fold.h); wpt_set_walk(WPT_WALK_NO_FOLD) keeps every node's own first child.  The walk is the same walk
with fewer steps, so every launch renders the same frame bit for bit with the fold and without it: the plain kernel and its
rotated and sliced twins, rays whose box tests take the NaN form, and the transient, time-of-flight, views and adaptive kernels.
The Cornell frames are the oracle's as well."""
import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def both(dev, launch, walk=0):
    """what `launch` returns with the fold (the default) and without it, and the kernel's name and form of each"""
    out = []
    try:
        for flags in (walk, walk | dev.WALK_NO_FOLD):
            dev.lib().wpt_set_walk(flags)
            got = launch()
            out.append((got, dev.lib().wpt_kernel_name().decode(), dev.lib().wpt_kernel_form().decode()))
    finally:
        dev.lib().wpt_set_walk(0)
    return out


@pytest.mark.parametrize("tall,short", [(1, 2), (0, 0)])
def test_cornell_frames_with_and_without_the_fold_are_the_oracles(dev, oracle, tall, short):
    sc = host.cornell(64, 64, tall, short)
    ds = dev.DeviceScene(sc)
    assert ds.folded_links() == dev.fold_plan(sc) == 6
    ref, _ = oracle.render(sc, 4)
    for walk in (0, dev.WALK_SELECT_CORNERS):                   # the rotated form and the form that selects the corners
        (on, name, form), (off, name_off, form_off) = both(dev, lambda: ds.render(4)[0], walk)
        assert name == name_off == "wpt_pathtrace" and form == form_off == ("" if walk else "rotated corners")
        assert bits_differing(on, off) == 0
        assert bits_differing(on, ref) == 0 and bits_differing(off, ref) == 0


def test_rays_whose_box_tests_take_the_nan_form(dev, oracle):
    """Pixel centres of an odd-sized frame seen along an axis: direction components of exactly zero, slab distances 0 * inf.  A
    random_triangles scene that fits LDS (its tree has no box twice: the fold must change nothing), and the Cornell box from
    its middle (six folded links)."""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    for sc in (host.random_triangles(100, 7, 33, 33, with_texcoords=False), host.cornell(33, 33, 1, 2)):
        assert sc.d.node_count * 32 + sc.d.tri_count * 48 <= 20 * 1024
        ds = dev.DeviceScene(sc)
        root = sc.d.nodes[0]
        lo, hi = np.array(root.lo[:], np.float64), np.array(root.hi[:], np.float64)
        mid = 0.5 * (lo + hi)
        saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
        try:
            for axis, sign in ((0, 1.0), (1, -1.0), (2, -1.0)):
                d = np.zeros(3)
                d[axis] = sign
                sc.camera[0] = host.camera_looking_at(sc, mid, mid + d, (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0))
                (on, name, _), (off, _, _) = both(dev, lambda: ds.render(2, params=p)[0])
                assert name == "wpt_pathtrace"
                assert bits_differing(on, off) == 0, (sc.name, axis)
                ref, _ = oracle.render(sc, 2, p)
                assert bits_differing(on, ref) == 0, (sc.name, axis)
        finally:
            sc.camera[0] = saved


def test_a_pooled_sliced_launch(dev):
    """more pixels than the device has lanes in flight: the pool hands them out, in two units of one row of strata each"""
    sc = host.cornell(640, 512, 1, 2)
    ds = dev.DeviceScene(sc)
    try:
        dev.set_slices(2)
        (on, _, form), (off, _, form_off) = both(dev, lambda: ds.render(2)[0])
    finally:
        dev.set_slices(0)
    assert form == form_off == "rotated corners, sliced x2"
    assert on.any() and bits_differing(on, off) == 0


def test_transient_tof_views_and_adaptive_launches(dev):
    sc = host.cornell(64, 64, 1, 2)
    ds = dev.DeviceScene(sc)
    edges = dev.uniform_edges(0.0, 1.0, 8)

    def transient():
        frame, bins = ds.render_transient(3, edges)
        return np.concatenate([frame[None], bins])
    (on, name, _), (off, name_off, _) = both(dev, transient)
    assert name == name_off == "wpt_pathtrace, transient, scene in LDS"
    assert on[1:].any() and bits_differing(on, off) == 0

    sensor = host.tof_sensor(contrast=0.75)
    (on, name, _), (off, name_off, _) = both(dev, lambda: ds.render_tof(3, sensor))
    assert name == name_off == "wpt_pathtrace, time of flight, scene in LDS"
    assert on.any() and bits_differing(on, off) == 0

    cams = [_abi.Camera.from_buffer_copy(sc.camera.contents),
            host.camera_looking_at(sc, (0.3, 1.2, 2.9), (0.0, 0.9, 0.0))]
    (on, name, _), (off, name_off, _) = both(dev, lambda: ds.render_views(3, cams).cpu().numpy())
    assert name == name_off == "wpt_pathtrace, views, scene in LDS"
    assert on[1].any() and bits_differing(on, off) == 0

    counts = (np.arange(64 * 64, dtype=np.int64).reshape(64, 64) % 5).astype(np.uint16)   # 0 .. 4 rows of strata per pixel

    def adaptive():
        frame, moments = ds.render_adaptive(counts, with_moments=True)
        return np.stack([frame.cpu().numpy(), moments.cpu().numpy()])
    (on, name, _), (off, name_off, _) = both(dev, adaptive)
    assert name == name_off == "wpt_pathtrace, adaptive, scene in LDS"
    assert on.any() and bits_differing(on, off) == 0
