"""The image operations on the GPU (wpt_k_image_ops.hip): the device forms give the host twins' bits and the reference's
(tests/golden/image_ops/) on every fixture case, on seeded random images, on sizes around the workgroup's tile, in both of
despeckle's forms, on a stream of their own, and on an OpenCV lens whose inverse takes one iteration in one lane and the most
in another of the same wave; the inputs stay as they were; and the distances of a ground truth pass come back as its positions."""
import numpy as np
import pytest
import torch

from tests import image_ops_cases as cases
from wurblpt_amd import device, host

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def _all_ops(image_c, rgb, camera, new_size, stream=None):
    """every operation on the device and on the host: [(what, device result as numpy, host result)]"""
    extra = {"stream": stream}
    d_image, d_rgb = _dev(image_c), _dev(rgb)
    got = [("resample", device.resample(d_image, *new_size, **extra), device.resample_host(image_c, *new_size))]
    for forward in (False, True):
        got.append(("warp forward=%d" % forward, device.lens_warp(d_image, camera, forward, **extra), device.lens_warp_host(image_c, camera, forward)))
    for pmd in (False, True):
        got.append(("coords pmd=%d" % pmd, device.distance_to_coords(d_image, camera, pmd, **extra), device.distance_to_coords_host(image_c, camera, pmd)))
    for factor in (1.0, 1.25):
        got.append(("despeckle %g" % factor, device.despeckle(d_rgb, factor, **extra), device.despeckle_host(rgb, factor)))
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    # the inputs are left as they were
    assert cases.same_bits(d_image.cpu().numpy(), image_c) and cases.same_bits(d_rgb.cpu().numpy(), rgb)
    return [(what, d.cpu().numpy(), h) for what, d, h in got]


@pytest.mark.parametrize("name", cases.names())
def test_device_form_gives_the_host_twins_and_the_references_bits(name):
    c = cases.case(name)
    image = np.ascontiguousarray(cases.image_of(c))
    d_image = _dev(image)
    got = cases.run(c, d_image, on_device=True).cpu().numpy()
    assert cases.same_bits(got, cases.run(c, image, on_device=False)), name
    assert cases.same_bits(got, cases.expected_of(c)), name
    assert cases.same_bits(d_image.cpu().numpy(), image)


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (5, 3), (33, 9), (130, 70)])
@pytest.mark.parametrize("lens", ["none", "radial_and_planar", "radial_only", "opencv"])
def test_seeded_random_images(size, lens):
    w, h = size
    comps = 1 + (w + list(cases.LENSES).index(lens)) % 4
    image = cases.seeded(w, h, comps, 100 + w, 0.5, 4.0)
    rgb = cases.fireflies(w, h, 200 + w)
    for what, got, want in _all_ops(image, rgb, cases.lens(lens), (h + 3, w + 2)):
        assert cases.same_bits(got, want), (what, size, lens)


def test_sizes_around_the_workgroups_tile_and_both_forms_of_despeckle():
    tw, th = device.image_ops_tile()
    camera = cases.lens("opencv")
    try:
        for w in (tw - 1, tw, tw + 1):
            for h in (th - 1, th, th + 1):
                image = cases.seeded(w, h, 3, 7 * w + h)
                rgb = cases.fireflies(w, h, 11 * w + h)
                for what, got, want in _all_ops(image, rgb, camera, (tw + (w - tw) * 2, th + (h - th) * 2)):
                    assert cases.same_bits(got, want), (what, w, h)
                # two tiles and a bit in each direction, both forms of despeckle
                big = cases.fireflies(2 * w + 1, 2 * h + 1, 13 * w + h)
                want = device.despeckle_host(big, 1.25)
                assert not cases.same_bits(want, big)
                for form in (0, 1):
                    device.set_despeckle_form(form)
                    assert device.despeckle_form() == ("gather", "tile")[form]
                    assert cases.same_bits(device.despeckle(_dev(big), 1.25).cpu().numpy(), want), (form, w, h)
                    assert cases.same_bits(device.despeckle(_dev(rgb), 1.25).cpu().numpy(), device.despeckle_host(rgb, 1.25)), (form, w, h)
                device.set_despeckle_form(-1)
    finally:
        device.set_despeckle_form(-1)


def test_on_a_stream_of_its_own():
    stream = torch.cuda.Stream()
    image = cases.seeded(70, 41, 4, 5)
    rgb = cases.fireflies(70, 41, 6)
    for what, got, want in _all_ops(image, rgb, cases.lens("radial_and_planar"), (33, 90), stream=stream):
        assert cases.same_bits(got, want), what


def _opencv_iterations(p, q, cam, width, height):
    """how many steps LensDistortion::undistort's OpenCV iteration takes at (p, q), in float32 (wpt_lens.h)"""
    f = np.float32
    cx, cy = (f(v) for v in cam.dist_center)
    ifx, ify = (f(v) for v in cam.dist_inverse_focal_length)
    fx, fy = (f(v) for v in cam.dist_focal_length)
    k1, k2, k3, p1, p2 = (f(v) for v in (cam.k1, cam.k2, cam.k3, cam.p1, cam.p2))

    def distort(p, q):
        s, t = (p - cx) * ifx, (q - cy) * ify
        r2 = s * s + t * t
        r4 = r2 * r2
        rd = f(1) + k1 * r2 + k2 * r4 + k3 * (r4 * r2)
        t1, t2, t3 = f(2) * s * t, r2 + f(2) * s * s, r2 + f(2) * t * t
        return (s * rd + p1 * t1 + p2 * t2) * fx + cx, (t * rd + p1 * t3 + p2 * t1) * fy + cy

    s, t = (p - cx) * ifx, (q - cy) * ify
    s0, t0, err, n = s, t, f(3.4e38), 0
    while n < 256 and err >= f(0.001) * f(0.001):
        r2 = s * s + t * t
        r4 = r2 * r2
        inv = f(1) / (f(1) + k1 * r2 + k2 * r4 + k3 * (r4 * r2))
        ds = f(2) * p1 * s * t + p2 * (r2 + f(2) * s * s)
        dt = f(2) * p2 * s * t + p1 * (r2 + f(2) * t * t)
        s, t = (s0 - ds) * inv, (t0 - dt) * inv
        ep, eq = distort(s * fx + cx, t * fy + cy)
        ox, oy = (ep - p) * f(width), (eq - q) * f(height)
        err = ox * ox + oy * oy
        n += 1
    return n


def test_opencv_inverse_of_one_and_of_many_iterations_in_one_wave():
    """33 x 3, a symmetric frustum and k1 = -0.2: in the middle row the centre pixel lies on the principal point and converges
    at once, the pixels at the left edge never do (256 steps); both lie in the first wave of the first workgroup"""
    w, h = 33, 3
    tw, th = device.image_ops_tile()
    assert tw * 2 >= 64 and th >= 2
    cam = host.lens_camera((-1.0, 1.0, -3.0 / 33.0, 3.0 / 33.0), 3, k1=-0.2)
    with np.errstate(all="ignore"):
        steps = [_opencv_iterations(np.float32(x + 0.5) * (np.float32(1) / np.float32(w)), np.float32(1.5) * (np.float32(1) / np.float32(h)), cam, w, h)
                 for x in range(32)]
    assert min(steps) == 1 and max(steps) == 256 and sorted(set(steps))[1] > 1, steps
    image = cases.seeded(w, h, 3, 9)
    got = device.lens_warp(_dev(image), cam, True).cpu().numpy()
    assert cases.same_bits(got, device.lens_warp_host(image, cam, True))
    assert np.isfinite(got).all()


def test_distances_of_a_ground_truth_pass_come_back_as_its_positions():
    """One chain without leaving the device: the camera space distances of a first-hit pass through distance_to_coords against its
    camera space positions where something is hit.  A plumbing check of signs, centre and focal length: a half-pixel shift or a
    flipped axis is off by at least 0.5 / 64 of the frustum's width, about 5e-3 of |P|; float rounding is near 1e-6; the bound
    2^-14 |P| lies two orders from either (tests/test_image_ops_host.py checks the same margin on an analytic plane)."""
    scene = host.cornell(64, 64)
    assert scene.camera.contents.distortion_type == 0 and scene.camera.contents.lens_radius == 0.0
    dscene = device.DeviceScene(scene)
    bits = sum(1 << device.GT_NAMES.index(n) for n in ("camera_space_positions", "camera_space_distances", "materials"))
    gt = dscene.ground_truth_device(bits)
    coords = device.distance_to_coords(gt["camera_space_distances"], scene.camera.contents)
    pmd = device.distance_to_coords(gt["camera_space_distances"], scene.camera.contents, pmd_space=True)
    torch.cuda.synchronize()
    dscene.check()
    P = gt["camera_space_positions"].cpu().numpy().astype(np.float64)
    hit = gt["materials"].cpu().numpy().reshape(64, 64) >= 0
    got = coords.cpu().numpy().astype(np.float64)
    assert hit.sum() > 64 * 64 // 2
    err = np.sqrt(((got - P) ** 2).sum(axis=2))[hit] / np.sqrt((P * P).sum(axis=2))[hit]
    print("cornell 64 x 64: largest error %.3g of |P| over %d pixels" % (err.max(), hit.sum()))
    assert err.max() <= 2.0 ** -14
    flipped = pmd.cpu().numpy().astype(np.float64)
    assert np.array_equal(flipped[..., 0], got[..., 0]) and np.array_equal(flipped[..., 1], -got[..., 1]) and np.array_equal(flipped[..., 2], -got[..., 2])
