"""The kernel with the scene in LDS in its two forms: corners held in all three rotations of (x, y, z) and read in the ray's
component order (the default where the copies leave four workgroups per compute unit; wpt_kernel_form() says "rotated corners"),
and the form that selects the components by the ray's axes (wpt_set_walk(WPT_WALK_SELECT_CORNERS)).  Both render the oracle's
frame bit for bit, for the Cornell box with every kind of box material, seen along every axis in both directions from inside the
box (camera rays of every kz and both signs; scattered and light rays take every direction anyway); a scene that fits LDS but
not with the copies keeps the select form."""
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
    assert a.shape == b.shape
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def render_both(dev, ds, s, params=None):
    """(frame, form) of the default launch and of the launch that keeps the select form"""
    try:
        dev.lib().wpt_set_walk(0)
        rot, _ = ds.render(s, params=params)
        rot_name, rot_form = dev.lib().wpt_kernel_name(), dev.lib().wpt_kernel_form()
        dev.lib().wpt_set_walk(dev.WALK_SELECT_CORNERS)
        sel, _ = ds.render(s, params=params)
        sel_name, sel_form = dev.lib().wpt_kernel_name(), dev.lib().wpt_kernel_form()
    finally:
        dev.lib().wpt_set_walk(0)
    assert rot_name == b"wpt_pathtrace" and sel_name == b"wpt_pathtrace"
    return rot, rot_form, sel, sel_form


def axis_cameras(sc):
    """the scene's own camera, then cameras at the middle of the scene's box looking along +x, -x, +y, -y, +z, -z"""
    root = sc.d.nodes[0]
    lo, hi = np.array(root.lo[:], np.float64), np.array(root.hi[:], np.float64)
    mid = 0.5 * (lo + hi) + 0.013 * (hi - lo)   # a little off the middle: no ray runs along a plane of symmetry
    cams = [("scene", _abi.Camera.from_buffer_copy(sc.camera.contents))]
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3)
            d[axis] = sign
            up = (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0)
            cams.append(("%s%s" % ("+" if sign > 0 else "-", "xyz"[axis]), host.camera_looking_at(sc, mid, mid + d, up)))
    return cams


@pytest.mark.parametrize("tall,short", [(0, 0), (1, 2), (1, 3)])
def test_both_forms_render_the_oracles_frame(dev, oracle, tall, short):
    sc = host.cornell(48, 40, tall, short)
    ds = dev.DeviceScene(sc)
    saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
    try:
        for label, cam in axis_cameras(sc):
            sc.camera[0] = cam
            ref, _ = oracle.render(sc, 3)
            rot, rot_form, sel, sel_form = render_both(dev, ds, 3)
            assert rot_form == b"rotated corners" and sel_form == b"", (label, rot_form, sel_form)
            assert np.isfinite(ref).all() and ref.any(), label
            assert bits_differing(rot, ref) == 0, (label, "rotated corners", bits_differing(rot, ref))
            assert bits_differing(sel, ref) == 0, (label, "select form", bits_differing(sel, ref))
    finally:
        sc.camera[0] = saved


def test_blocks_and_the_pixel_pool(dev, oracle):
    """a frame large enough for the pixel pool, and a ragged block of it"""
    sc = host.cornell(512, 384, 1, 2)
    ds = dev.DeviceScene(sc)
    ref, _ = oracle.render(sc, 1)
    rot, rot_form, sel, sel_form = render_both(dev, ds, 1)
    assert rot_form == b"rotated corners" and sel_form == b""
    assert bits_differing(rot, ref) == 0 and bits_differing(sel, ref) == 0
    start, size = 1037, 512 * 384 - 5001
    part, _ = ds.render(1, block=(start, size))
    assert dev.lib().wpt_kernel_form() == b"rotated corners"
    assert bits_differing(part.reshape(-1, 3)[start:start + size], ref.reshape(-1, 3)[start:start + size]) == 0
    assert not part.reshape(-1, 3)[:start].any() and not part.reshape(-1, 3)[start + size:].any()


def test_a_scene_too_large_for_the_copies_keeps_the_select_form(dev, oracle):
    """nodes and corners fit the LDS kernel's 20 KiB, but two more copies of the corners would not leave four workgroups per
    compute unit: the launch reports the old kernel"""
    sc = host.random_triangles(100, 7, 48, 40, with_texcoords=False)
    scene_bytes = sc.d.node_count * 32 + sc.d.tri_count * 48
    assert scene_bytes <= 20 * 1024                                                # it runs in the LDS kernel
    assert 33280 + scene_bytes + 32 + 2 * sc.d.tri_count * 48 > 160 * 1024 // 4    # and the copies do not fit beside it
    ds = dev.DeviceScene(sc)
    ref, _ = oracle.render(sc, 2)
    got, _ = ds.render(2)
    assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace" and dev.lib().wpt_kernel_form() == b""
    assert bits_differing(got, ref) == 0


def test_other_launches_of_the_cornell_box_keep_their_kernels(dev):
    """counting launches, batches of views, transient and adaptive launches and the wavefront form do not take the rotated form,
    and every one of them renders the plain frame"""
    sc = host.cornell(48, 40, 1, 2)
    ds = dev.DeviceScene(sc)
    plain, _ = ds.render(2)
    assert dev.lib().wpt_kernel_form() == b"rotated corners"
    counted, counters = ds.render(2, with_counters=True)
    assert dev.lib().wpt_kernel_form() == b"" and counters["rays"] > 0
    assert bits_differing(plain, counted) == 0
    views = ds.render_views(2, [_abi.Camera.from_buffer_copy(sc.camera.contents)]).cpu().numpy()
    assert dev.lib().wpt_kernel_form() == b"" and bits_differing(views[0], plain) == 0
    ds.render(2)
    assert dev.lib().wpt_kernel_form() == b"rotated corners"
    frame, _ = ds.render_transient(2, dev.uniform_edges(0.0, 1.0, 8))
    assert b"transient" in dev.lib().wpt_kernel_name() and dev.lib().wpt_kernel_form() == b""
    assert bits_differing(frame, plain) == 0
    ds.render(2)
    assert dev.lib().wpt_kernel_form() == b"rotated corners"
    adaptive = ds.render_adaptive(np.full((sc.height, sc.width), 2, dtype=np.uint16)).cpu().numpy()
    assert b"adaptive" in dev.lib().wpt_kernel_name() and dev.lib().wpt_kernel_form() == b""
    assert bits_differing(adaptive, plain) == 0
    ds.render(2)
    assert dev.lib().wpt_kernel_form() == b"rotated corners"
    try:
        dev.lib().wpt_set_wavefront(1, 0, 0, 0)
        wf, _ = ds.render(2)
        assert dev.lib().wpt_kernel_name() == b"wf_trace + wf_shade" and dev.lib().wpt_kernel_form() == b""
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert bits_differing(wf, plain) == 0
