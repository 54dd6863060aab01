"""The image operations (wpt_postproc_resample / _lens_warp / _despeckle / _distance_to_coords, wurblpt_amd/csrc/wpt_image_ops.h)
without a GPU: the entry points are exported and declared; the host forms give the bits of the reference's own functions
(tests/golden/image_ops/); bad calls are refused before a device is needed; the C++ interface compiled from the source that made
the fixtures writes them again byte for byte; wpt_image_ops.h stands on its own under the sanitizers and the library's host
entries reproduce its digests; extractComponent(s) copy components; and a distance image made from analytic positions on a plane
comes back as those positions."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import image_ops_cases as cases
from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
NEW = ("wpt_postproc_resample", "wpt_postproc_lens_warp", "wpt_postproc_despeckle", "wpt_postproc_distance_to_coords")


def test_entry_points_are_exported_and_declared():
    L = device.lib()
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    for name in [n + s for n in NEW for s in ("", "_host")] + ["wpt_postproc_despeckle_form", "wpt_set_despeckle_form", "wpt_postproc_image_ops_tile"]:
        assert name in device.EXPORTS and not re.search(r"\d", name)
        getattr(L, name)
        assert re.search(r"\b%s\(" % name, header)
    assert "#define WPT_ABI_VERSION 5u" in header and _abi.WPT_ABI_VERSION == 5
    assert device.despeckle_form() in ("tile", "gather")
    tw, th = device.image_ops_tile()
    assert tw * th in (64, 128, 256, 512, 1024)
    unit = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read()
    assert "wpt_k_image_ops" in unit.split()


def test_the_fixtures_cover_the_cases():
    index, data = cases.load()
    names = cases.names()
    assert len(set(names)) == len(names) and {c["op"] for c in index} == set(cases.OPS)
    for comps in (1, 2, 3, 4):
        for size in ("11x3", "7x5", "1x1", "3x13", "1x1_to_4x4"):
            assert "resample_c%d_%s" % (comps, size) in names
    for lens in cases.LENSES:
        for way in ("forward", "back"):
            assert "warp_%s_%s" % (lens, way) in names
    for frame in ("1x1", "1x7", "5x3", "constant", "speckles", "tie", "tie_swapped"):
        for f in range(3):
            assert "despeckle_%s_f%d" % (frame, f) in names
    for comps in (1, 3):
        for lens in ("none", "opencv"):
            for pmd in ("", "_pmd"):
                assert "coords_c%d_%s%s" % (comps, lens, pmd) in names
    assert max(max(c["w"], c["h"], c["out_w"], c["out_h"]) for c in index) <= 33
    assert data.nbytes < 100 * 1024 and all(c["out"] + c["out_w"] * c["out_h"] * c["out_c"] <= data.size for c in index)
    # the tie: the two frames differ in two pixels' last bits only, and the outputs' centres are the two different colours
    a, b = (cases.expected_of(cases.case("despeckle_tie%s_f1" % s))[1, 1] for s in ("", "_swapped"))
    assert not cases.same_bits(a, b)
    # some warped pixel of every lens differs from the plain resampling, and a two-component output repeats component 0
    plain = cases.expected_of(cases.case("warp_none_back"))
    for lens in ("radial_and_planar", "radial_only", "opencv"):
        assert not cases.same_bits(cases.expected_of(cases.case("warp_%s_back" % lens)), plain)
    two = cases.expected_of(cases.case("warp_opencv_back_c2"))
    assert cases.same_bits(two[..., 0], two[..., 1])


@pytest.mark.parametrize("name", cases.names())
def test_host_form_gives_the_references_bits(name):
    c = cases.case(name)
    image = cases.image_of(c)
    kept = image.copy()
    got = cases.run(c, image, on_device=False)
    assert cases.same_bits(got, cases.expected_of(c)), name
    assert cases.same_bits(image, kept)


def test_no_lens_still_resamples_and_is_not_a_copy_at_width_33():
    """WPT_DISTORTION_NONE resamples at the pixel centres; whether that equals a copy is a matter of rounding of (x + 0.5f) *
    (1.0f / width) * width - 0.5f, so the library does not shortcut it: the fixture decides, and at width 33 it is NOT a copy"""
    c = cases.case("warp_none_back")
    assert not cases.same_bits(cases.expected_of(c), cases.image_of(c))


def _call(name, host_form, *args):
    L = device.lib()
    fn = getattr(L, name + ("_host" if host_form else ""))
    st = fn(*args) if host_form else fn(*args, None)
    return st, L.wpt_last_error().decode()


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("host_form", [True, False])
def test_bad_calls_are_refused_before_a_device_is_needed(host_form):
    w, h = 6, 4
    img = cases.seeded(w, h, 3, 1)
    out = np.zeros((h, w, 3), np.float32)
    big = np.zeros((13, 11, 3), np.float32)
    cam = cases.lens("opencv")
    unknown = cases.lens("opencv")
    unknown.distortion_type = 4
    bad = []
    for name, tail in (("wpt_postproc_resample", lambda o: (11, 13, o)), ("wpt_postproc_lens_warp", lambda o: (C.byref(cam), 1, o)),
                       ("wpt_postproc_despeckle", lambda o: (C.c_float(1.25), o)),
                       ("wpt_postproc_distance_to_coords", lambda o: (C.byref(cam), 0, o))):
        o = _ptr(big if "resample" in name else out)
        bad += [(name, (None, w, h, 3) + tail(o), "NULL"), (name, (_ptr(img), w, h, 3) + tail(None), "NULL")]
        bad += [(name, (_ptr(img), ww, hh, 3) + tail(o), "width and height") for ww, hh in ((0, h), (w, 0), (65536, 1), (1, 65536))]
        bad += [(name, (_ptr(img), w, h, comps) + tail(o), "components") for comps in (0, 5)]
        bad += [(name, (_ptr(img), w, h, 3) + tail(_ptr(img)), "overlaps")]
        bad += [(name, (_ptr(img), w, h, 3) + tail(_ptr(img.reshape(-1)[w * h * 3 - 1:])), "overlaps")]
    bad += [("wpt_postproc_resample", (_ptr(img), w, h, 3, nw, nh, _ptr(big)), "width and height") for nw, nh in ((0, 3), (3, 0), (65536, 1), (1, 65536))]
    bad += [("wpt_postproc_despeckle", (_ptr(img), w, h, comps, C.c_float(1.25), _ptr(out)), "3 components") for comps in (1, 2, 4)]
    bad += [("wpt_postproc_despeckle", (_ptr(img), w, h, 3, C.c_float(f), _ptr(out)), "min_factor") for f in (math.inf, -math.inf, math.nan)]
    for name in ("wpt_postproc_lens_warp", "wpt_postproc_distance_to_coords"):
        bad += [(name, (_ptr(img), w, h, 3, None, 0, _ptr(out)), "camera is NULL"), (name, (_ptr(img), w, h, 3, C.byref(unknown), 0, _ptr(out)), "unknown distortion type")]
    assert len(bad) >= 50
    for name, args, what in bad:
        st, msg = _call(name, host_form, *args)
        assert st == INVALID_ARGUMENT and what in msg, (name, what, st, msg)
    if host_form:
        assert _call("wpt_postproc_resample", True, _ptr(img), w, h, 3, 11, 13, _ptr(big))[0] == 0
        assert _call("wpt_postproc_despeckle", True, _ptr(img), w, h, 3, C.c_float(1.25), _ptr(out))[0] == 0


def test_the_cpp_interface_writes_the_fixtures_again(tmp_path):
    """tests/image_ops_cases.cpp, the source that made tests/golden/image_ops/ over the reference's functions, built against
    include/: the drop-in at source level, and the same bytes"""
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "image_ops_cases")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include", "wurblpt"), os.path.join(ROOT, "tests", "image_ops_cases.cpp"), "-L" + lib,
                    "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
    for name in ("index.json", "data.bin"):
        assert open(str(tmp_path / name), "rb").read() == open(os.path.join(cases.GOLDEN, name), "rb").read(), name


def test_the_rules_on_their_own_under_the_sanitizers_and_their_digests(tmp_path):
    """tests/image_ops_check.cpp: wpt_image_ops.h without the library or a header of HIP, every buffer of the promised size; its
    digests are tests/golden/image_ops_digests.json's, and the library's host entries reproduce them from the inputs it leaves"""
    exe = str(tmp_path / "image_ops_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "image_ops_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:]
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "image_ops_digests.json")))
    assert json.loads(r.stdout.decode()) == golden
    digests = golden["digests"]
    assert golden["sizes"][0][:2] == [1, 1] and len(golden["sizes"]) == 10
    wild = {"far": (3, 3.0e6, 0.0, 0.0, 2.0e5, -1.0e5), "overflow": (3, 3.0e38, 3.0e38, 3.0e38, 3.0e38, -3.0e38)}
    lenses = {name: host.lens_camera(cases.FRUSTUM, *k) for name, k in list(cases.LENSES.items()) + list(wild.items())}
    count = 0
    for i, (w, h, comps, w2, h2) in enumerate(golden["sizes"]):
        image = np.fromfile(str(tmp_path / ("image_%d.bin" % i)), np.float32).reshape(h, w, comps)
        rgb = np.fromfile(str(tmp_path / ("rgb_%d.bin" % i)), np.float32).reshape(h, w, 3)
        assert cases.digest(device.resample_host(image, w2, h2)) == digests["resample_%d" % i]
        for name, cam in lenses.items():
            for forward in (False, True):
                got = device.lens_warp_host(image, cam, forward)
                assert cases.digest(got) == digests["warp_%s_%s_%d" % (name, "forward" if forward else "back", i)], (name, forward, i)
                count += 1
            if name in ("none", "opencv", "far", "overflow"):
                for pmd in (False, True):
                    got = device.distance_to_coords_host(image, cam, pmd)
                    assert cases.digest(got) == digests["coords_%s%s_%d" % (name, "_pmd" if pmd else "", i)], (name, pmd, i)
        for f, factor in enumerate((1.0, 1.25, 4.0)):
            assert cases.digest(device.despeckle_host(rgb, factor)) == digests["despeckle_f%d_%d" % (f, i)]
    assert count == 120


def test_extract_components_and_tags(tmp_path):
    src = tmp_path / "extract.cpp"
    src.write_text(r'''
#include <cstdio>
#include <wurblpt/postproc.hpp>
using namespace WurblPT;
int main()
{
    Array<float> a({ size_t(3), size_t(2) }, 4);
    for (size_t e = 0; e < a.elementCount(); e++)
        for (size_t c = 0; c < 4; c++)
            a[e][c] = float(10 * e + c);
    a.globalTagList().set("WURBLPT/TEST", "kept");
    const Array<float> two = extractComponents(a, { 3, 1 });
    const Array<float> one = extractComponent(a, 2);
    bool ok = two.componentCount() == 2 && one.componentCount() == 1 && two.dimension(0) == 3 && one.dimension(1) == 2
        && two.globalTagList().value("WURBLPT/TEST") == "kept";
    for (size_t e = 0; e < a.elementCount(); e++)
        ok = ok && two[e][0] == a[e][3] && two[e][1] == a[e][1] && one[e][0] == a[e][2];
    Array<uint8_t> bytes({ size_t(2), size_t(2) }, 3);
    bytes[{ size_t(1), size_t(1) }][2] = 77;
    ok = ok && Array<uint8_t>(extractComponent(bytes, 2))[3][0] == 77 && extractComponent(bytes, 2).componentType() == TGD::uint8;
    bool refused = false;
    try { extractComponent(a, 4); } catch (const std::invalid_argument&) { refused = true; }
    /* the image operations keep the tags and the component count, and cameraSpaceToPMDSpace negates y and z */
    const Array<float> s = scale(a, 5, 4), d = undistort(a, LensDistortion(0.1f, 0.0f, 0.0f), Projection());
    ok = ok && s.dimension(0) == 5 && s.dimension(1) == 4 && s.componentCount() == 4 && s.globalTagList().value("WURBLPT/TEST") == "kept";
    ok = ok && d.dimension(0) == 3 && d.componentCount() == 4 && d.globalTagList().value("WURBLPT/TEST") == "kept";
    const Array<float> pmd = cameraSpaceToPMDSpace(a);
    ok = ok && pmd.componentCount() == 3 && pmd[4][0] == a[4][0] && pmd[4][1] == -a[4][1] && pmd[4][2] == -a[4][2];
    bool rgbOnly = false;
    try { despeckle(a); } catch (const std::runtime_error&) { rgbOnly = true; }
    printf("%d %d %d\n", int(ok), int(refused), int(rgbOnly));
    return 0;
}
''')
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "extract")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib,
                    "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout.decode().split() == ["1", "1", "1"], r.stdout.decode() + r.stderr.decode()[-2000:]


def plane_distances(width, height, frustum):
    """camera space positions of the pixel centres' rays on the plane z = -3 - 0.5 x + 0.25 y (float64), and their lengths"""
    l, r, b, t = frustum
    y, x = np.mgrid[0:height, 0:width]
    u = l + (r - l) * (x + 0.5) / width
    v = b + (t - b) * (y + 0.5) / height
    # the ray s * (u, v, -1) meets the plane where -s = -3 - 0.5 s u + 0.25 s v
    s = 3.0 / (1.0 - 0.5 * u + 0.25 * v)
    P = np.stack([s * u, s * v, -s], axis=2)
    return P, np.sqrt((P * P).sum(axis=2))


def test_distances_of_a_plane_come_back_as_its_positions():
    """Signs, centre and focal length: a half-pixel shift or a flipped axis is off by at least 0.5 / 64 of the frustum's width,
    about 5e-3 of |P|; float rounding is near 1e-6; the bound 2^-14 |P| lies two orders from either"""
    w = h = 64
    frustum = (-0.5, 0.625, -0.4375, 0.5)
    P, dist = plane_distances(w, h, frustum)
    cam = host.lens_camera(frustum)
    got = device.distance_to_coords_host(dist.astype(np.float32), cam).astype(np.float64)
    err = np.sqrt(((got - P) ** 2).sum(axis=2)) / np.sqrt((P * P).sum(axis=2))
    print("plane: largest error %.3g of |P|" % err.max())
    assert err.max() <= 2.0 ** -14
    pmd = device.distance_to_coords_host(dist.astype(np.float32), cam, pmd_space=True).astype(np.float64)
    assert np.array_equal(pmd[..., 0], got[..., 0]) and np.array_equal(pmd[..., 1], -got[..., 1]) and np.array_equal(pmd[..., 2], -got[..., 2])
    # and the conventions the bound is there to catch do miss it
    shifted = np.roll(got, 1, axis=1)
    assert (np.sqrt(((shifted - P) ** 2).sum(axis=2)) / np.sqrt((P * P).sum(axis=2)))[:, 1:].min() > 2.0 ** -14
