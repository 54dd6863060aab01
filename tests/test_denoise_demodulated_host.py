"""The first-hit colour pass and the denoiser on the demodulated frame (wpt_first_hit_colours*, wpt_postproc_denoise_demodulated*;
wurblpt_amd/csrc/wpt_denoise.h) without a GPU: the entry points are exported and refuse bad calls before a device is needed; the
host form agrees with a float64 restatement of the rule written here from its description; with nothing to take out it is the
plain filter bit for bit; a constant light on a checker of albedos with emitters comes back untouched where the plain filter blurs
the checker; wpt_denoise.h's demodulated form stands on its own under the sanitizers and the library's host entry reproduces its
digests; the C++ interface gives the host form's bits."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_cases as cases
from tests.test_denoise_host import H, KY, _relative, _seeded_case, _shift, _uniform_guide
from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
FLOOR = 1.0 / 64
CHECKER = np.array([[0.9, 0.1, 0.5], [0.05, 0.8, 0.0]], np.float32)    # the second's blue lies below the floor
NEW = ("wpt_first_hit_colours_device", "wpt_first_hit_colours", "wpt_postproc_denoise_demodulated", "wpt_postproc_denoise_demodulated_host")


def test_entry_points_are_exported_and_declared():
    L = device.lib()
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    for name in NEW:
        assert name in device.EXPORTS
        getattr(L, name)
        assert re.search(r"\b%s\(" % name, header)
    for name in ("first_hit_colours", "denoise_demodulated", "denoise_demodulated_host"):
        assert callable(getattr(device, name))
    assert callable(device.DeviceScene.first_hit_colours_device)
    assert "#define WPT_ABI_VERSION 5u" in header and _abi.WPT_ABI_VERSION == 5
    assert _abi.DENOISE_ALBEDO_FLOOR == FLOOR
    assert C.sizeof(_abi.DenoiseParams) == 16                      # the parameters keep their layout: the floor is an argument
    unit = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read()
    assert "wpt_k_firsthit" in unit.split() and os.path.exists(os.path.join(ROOT, "wurblpt_amd", "csrc", "wpt_k_firsthit.hip"))


def checker(w, h, cell=4):
    y, x = np.mgrid[0:h, 0:w]
    return CHECKER[((x // cell + y // cell) % 2)]


def seeded_colours(frame, seed=11):
    """the checker of albedos, and an emission in a tenth of the pixels: between a quarter and three quarters of what the frame
    holds there, so that u stays positive and the remodulated sum does not cancel (float against float64 stays well conditioned)"""
    h, w = frame.shape[:2]
    rng = np.random.RandomState(seed)
    emits = rng.rand(h, w) < 0.1
    emission = np.where(emits[..., None], frame * (0.25 + 0.5 * rng.rand(h, w, 3)), 0).astype(np.float32)
    assert emission.any()
    return checker(w, h), emission


def _call(host_form, arrays, width, height, params, floor, out, variance):
    L = device.lib()
    ptr = [None if a is None else C.c_void_p(a.ctypes.data) for a in arrays + [out, variance]]
    p = None if params is None else C.byref(params)
    if host_form:
        st = L.wpt_postproc_denoise_demodulated_host(*ptr[:8], width, height, p, floor, ptr[8], ptr[9])
    else:
        st = L.wpt_postproc_denoise_demodulated(*ptr[:8], width, height, p, floor, ptr[8], ptr[9], None)
    return st, L.wpt_last_error().decode()


@pytest.mark.parametrize("host_form", [True, False])
def test_bad_denoiser_calls_are_refused_before_a_device_is_needed(host_form):
    w, h = 6, 4
    c = cases.inputs(w, h)
    albedo, emission = seeded_colours(c["frame"])
    albedo = np.ascontiguousarray(albedo)
    good = [c["frame"], c["moments"], c["samples_sqrt"], c["positions"], c["normals"], c["materials"], albedo, emission]
    out = np.zeros((h, w, 3), np.float32)
    var = np.zeros((h, w), np.float32)
    P = _abi.DenoiseParams
    bad = [(good[:k] + [None] + good[k + 1:], w, h, P(), 0.0, out, var, "NULL") for k in range(8)]
    bad += [(good, w, h, P(), floor, out, var, "albedo_floor") for floor in (math.nan, math.inf, -math.inf)]
    bad += [(good, w, h, P(), 0.0, None, var, "output frame is NULL")]
    bad += [(good, ww, hh, P(), 0.0, out, var, "width and height") for ww, hh in ((0, h), (w, 0), (65536, 1), (1, 65536))]
    bad += [(good, w, h, P(iterations=9), 0.0, out, var, "iterations"), (good, w, h, P(normal_log2=17), 0.0, out, var, "normal_log2")]
    bad += [(good, w, h, P(sigma_l=s), 0.0, out, var, "sigma") for s in (0.0, -1.0, math.inf, math.nan)]
    bad += [(good, w, h, P(sigma_z=s), 0.0, out, var, "sigma") for s in (0.0, -0.1, math.inf, math.nan)]
    bad += [(good, w, h, P(), 0.0, good[k], var, "aliases") for k in (0, 1, 3, 4, 6, 7)]
    bad += [(good, w, h, P(), 0.0, out, good[5].view(np.float32), "aliases"), (good, w, h, P(), 0.0, out, out.reshape(-1)[7:7 + w * h], "aliases")]
    bad += [(good, w, h, P(), 0.0, out, good[k].reshape(-1)[5:5 + w * h], "aliases") for k in (6, 7)]
    for arrays, ww, hh, params, floor, o, v, what in bad:
        st, msg = _call(host_form, arrays, ww, hh, params, floor, o, v)
        assert st == INVALID_ARGUMENT and "denoise" in msg and what in msg, (what, st, msg)
    if host_form:   # the good call passes: the defaults for no parameters, no variance plane, a floor of its own and the default's sign
        for params, floor, v in ((None, 0.0, None), (P(), -1.0, var), (P(), 0.3, var)):
            assert _call(True, good, w, h, params, floor, out, v)[0] == 0
            assert np.isfinite(out).all() and np.isfinite(var).all()


@pytest.mark.parametrize("host_form", [True, False])
def test_bad_first_hit_calls_are_refused_before_a_device_is_needed(host_form):
    L = device.lib()
    w, h = 5, 3
    scene = C.create_string_buffer(4096)            # never read: every refusal comes before the scene is looked at
    camera, params = _abi.Camera(), host.default_params()
    albedo, emission, P, n = (np.zeros((h, w, 3), np.float32) for _ in range(4))
    m = np.zeros((h, w), np.int32)

    def call(scene, camera, params, ww, hh, albedo, emission, guide):
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        g = None if guide is None else (C.c_void_p * 3)(*[None if a is None else a.ctypes.data for a in guide])
        args = [None if scene is None else C.addressof(scene), None if camera is None else C.addressof(camera),
                None if params is None else C.addressof(params), ww, hh, ptr(albedo), ptr(emission), g]
        st = L.wpt_first_hit_colours(*args) if host_form else L.wpt_first_hit_colours_device(*args, None)
        return st, L.wpt_last_error().decode()

    guide = (P, n, m)
    bad = [(None, camera, params, w, h, albedo, emission, guide, "NULL"), (scene, None, params, w, h, albedo, emission, guide, "NULL"),
           (scene, camera, None, w, h, albedo, emission, guide, "NULL")]
    bad += [(scene, camera, params, ww, hh, albedo, emission, guide, "width and height") for ww, hh in ((0, h), (w, 0), (65536, 1), (1, 65536))]
    bad += [(scene, camera, params, w, h, None, None, g, "no output") for g in (None, (None, None, None))]
    flat = np.zeros(w * h * 3 + 7, np.float32)
    bad += [(scene, camera, params, w, h, albedo, albedo, guide, "overlap"), (scene, camera, params, w, h, albedo, emission, (P, P, m), "overlap"),
            (scene, camera, params, w, h, albedo, emission, (albedo, n, m), "overlap"),
            (scene, camera, params, w, h, flat[:w * h * 3], flat[7:], None, "overlap"),
            (scene, camera, params, w, h, None, emission, (None, None, emission.view(np.int32).reshape(-1)[5:5 + w * h]), "overlap")]
    for *args, what in bad:
        st, msg = call(*args)
        assert st == INVALID_ARGUMENT and "first-hit colours" in msg and what in msg, (what, st, msg)


def reference(frame, moments, n_p, P, n, m, albedo, emission, floor=FLOOR, sigma_l=1.0, sigma_z=0.1, normal_log2=7, iterations=5):
    """The rule as its description states it, in float64: demodulate, the iterations of the plain filter, remodulate; returns the
    frame and the variance plane (of the demodulated luminance)."""
    f, mo, P, n, al, em = (a.astype(np.float64) for a in (frame, moments, P, n, albedo, emission))
    d = np.where(al >= floor, al, 1.0)
    u = (f - em) / d
    N = n_p.astype(np.float64) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where((n_p >= 2)[..., None], np.maximum(mo - f * f, 0) / (N - 1)[..., None] / (d * d), u * u)
    V = (np.sqrt(v) @ KY) ** 2
    c = u
    sky = m < 0
    for i in range(iterations):
        s = 2 ** i
        gs, gw = np.zeros_like(V), np.zeros_like(V)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Vq, valid = _shift(V, dx, dy)
                k = (2 - abs(dx)) * (2 - abs(dy))
                gs += np.where(valid, k * Vq, 0)
                gw += np.where(valid, k, 0)
        L = sigma_l * np.sqrt(gs / gw) + 1e-10
        sw, sc, sv = np.zeros_like(V), np.zeros_like(c), np.zeros_like(V)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                mq, valid = _shift(m, s * dx, s * dy)
                nq, Pq, cq, Vq = (_shift(a, s * dx, s * dy)[0] for a in (n, P, c, V))
                wn = np.maximum(0, (n * nq).sum(axis=2)) ** (2 ** normal_log2)
                D = Pq - P
                t, dd = (n * D).sum(axis=2), (D * D).sum(axis=2)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ez = np.where(dd == 0, 0, t * t / (sigma_z * sigma_z * dd))
                wn, ez = np.where(sky, 1, wn), np.where(sky, 0, ez)
                el = np.abs(cq @ KY - c @ KY) / L
                w = np.where(valid & (mq == m), H[dy + 2] * H[dx + 2] * wn * np.exp(-(ez + el)), 0)
                sw += w
                sc += w[..., None] * cq
                sv += w * w * Vq
        c, V = sc / sw[..., None], sv / (sw * sw)
    return c * d + em, V


@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
def test_host_form_is_the_rule_in_float64(iterations):
    c = _seeded_case()
    albedo, emission = seeded_colours(c["frame"])
    assert (albedo < FLOOR).any() and 0.05 < (emission.any(axis=2)).mean() < 0.2
    got, var = device.denoise_demodulated_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), albedo, emission,
                                               _abi.DenoiseParams(iterations=iterations), 0.0, True)
    want, want_var = reference(c["frame"], c["moments"], c["samples_sqrt"], *cases.guide(c), albedo, emission, iterations=iterations)
    print("iterations %d: colour %.3g, variance %.3g relative" % (iterations, _relative(got, want), _relative(var, want_var)))
    assert _relative(got, want) <= 1e-4 and _relative(var, want_var) <= 1e-4
    # another floor is another rule: 0.3 leaves the checker's 0.1 and 0.05 alone as well
    got3 = device.denoise_demodulated_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), albedo, emission,
                                           _abi.DenoiseParams(iterations=iterations), 0.3)
    want3, _ = reference(c["frame"], c["moments"], c["samples_sqrt"], *cases.guide(c), albedo, emission, floor=0.3, iterations=iterations)
    assert _relative(got3, want3) <= 1e-4
    assert iterations == 0 or not np.array_equal(got3, got)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("albedo_value", [1.0, FLOOR / 2], ids=["albedo_one", "albedo_below_floor"])
def test_with_nothing_to_take_out_it_is_the_plain_filter(kind, albedo_value):
    """albedo 1 (d = 1), or an albedo below the floor in every channel (d = 1 again), and no emission: x - 0, x / 1, x * 1 and
    x + 0 are x for the non-negative frames of these cases, so the output and the variance are wpt_postproc_denoise_host's bits"""
    for w, h in cases.SIZES:
        c = cases.inputs(w, h, kind)
        albedo = np.full((h, w, 3), albedo_value, np.float32)
        emission = np.zeros((h, w, 3), np.float32)
        for iterations in (0, 1, 5, 8) if w * h > 100 else range(9):
            p = _abi.DenoiseParams(iterations=iterations)
            want, want_var = device.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), p, True)
            got, var = device.denoise_demodulated_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), albedo, emission, p, 0.0, True)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(var.view(np.uint32), want_var.view(np.uint32)), (w, h, iterations)


def _constant_light_frame(w, h):
    albedo = checker(w, h)
    rng = np.random.RandomState(3)
    light = np.array([1.5, 1.0, 0.75], np.float32)
    emission = np.where((rng.rand(h, w) < 0.1)[..., None], rng.rand(h, w, 3) * 2, 0).astype(np.float32)
    frame = (albedo * light + emission).astype(np.float32)
    return albedo, emission, light, frame


def _bound(frame, emission, iterations):
    """|out - frame| of a pixel whose filtered u is a mean of u's that are equal but for their rounding, eps = 2^-24:
      the four operations   s = frame - e, u = s / d, c * d, + e: each rounds its result by eps relative, and the results are at
                            most |frame| + |e| in size: 4 eps (|frame| + max e)
      the u's of the taps   pixels of one albedo hold one true u, but an emitter's frame was rounded with its emission in it, and
                            its u again by the two operations: d * |u_q - u_p| <= 4 eps (|frame| + max e)
      an iteration          sum(w u) / sum(w) over at most 25 taps of one sign: 24 additions and a product above, 24 additions
                            below (an error of w itself cancels between the two), one division: 50 eps relative
    """
    eps = 2.0 ** -24
    size = np.abs(frame.astype(np.float64)) + float(emission.max())
    return eps * (8 + 50 * iterations) * size


def test_a_constant_light_on_a_checker_of_albedos_comes_back():
    """frame = albedo * L + emission with one L, one material, n_p = 5 and the moments of a noise-free pixel (moment = frame^2,
    channel variance 0): the demodulated frame is L everywhere (0 in the channel whose albedo lies below the floor, where the
    texture stays in u), and the filter returns it.

    Of the plain filter the issue expects that it moves THIS frame by more than a tenth of the checker's contrast.  It does not:
    with a variance of 0 the luminance tolerance is 1e-10, every tap on the other albedo weighs exp(-1e9) = 0, and the plain
    filter returns the frame as well (asserted below, so that the record is right).  What is gained shows on the same frame once
    the moments say what a noisy light says -- see the next test."""
    w, h = 40, 24
    albedo, emission, light, frame = _constant_light_frame(w, h)
    moments = (frame * frame).astype(np.float32)
    guide = _uniform_guide(w, h)
    for iterations in (1, 5):
        p = _abi.DenoiseParams(iterations=iterations)
        got = device.denoise_demodulated_host(frame, moments, 5, guide, albedo, emission, p)
        err = np.abs(got.astype(np.float64) - frame)
        print("%d iterations: largest error %.3g, %.3g of its bound" % (iterations, err.max(), (err / _bound(frame, emission, iterations)).max()))
        assert (err <= _bound(frame, emission, iterations)).all()
        plain = device.denoise_host(frame, moments, 5, guide, p)
        assert (np.abs(plain.astype(np.float64) - frame) <= _bound(frame, emission, iterations)).all()


def test_under_a_noisy_light_the_plain_filter_blurs_the_checker_and_the_demodulated_one_does_not():
    """The same frame, its moments those of a light with the standard deviation L / 2 per sample on noise-free surface colours:
    the channel variance is (albedo * L / 2)^2 / 25.  The plain filter now takes the checker's contrast for noise and moves the
    pixels at the cells' edges by more than a tenth of it.  The demodulated frame is still L in every channel whose albedo
    clears the floor in both cells (red and green), and those come back within the same bound; blue, below the floor in one
    cell, is filtered as radiance there -- that is the rule, and it is left out of the comparison."""
    w, h = 40, 24
    albedo, emission, light, frame = _constant_light_frame(w, h)
    N = 25
    sigma = albedo.astype(np.float64) * light / 2
    moments = (frame.astype(np.float64) ** 2 + (N - 1) * sigma ** 2 / N).astype(np.float32)   # channelVariance gives sigma^2 / N back
    guide = _uniform_guide(w, h)
    p = _abi.DenoiseParams()
    got = device.denoise_demodulated_host(frame, moments, 5, guide, albedo, emission, p)
    err = np.abs(got.astype(np.float64) - frame)[..., :2]
    # the moment's own rounding leaves the variance estimate, not u: the bound is the one above
    print("largest error in red and green %.3g, %.3g of its bound" % (err.max(), (err / _bound(frame, emission, 5)[..., :2]).max()))
    assert (err <= _bound(frame, emission, 5)[..., :2]).all()
    plain = device.denoise_host(frame, moments, 5, guide, p)
    contrast = np.abs(CHECKER[0].astype(np.float64) - CHECKER[1]) * light
    y, x = np.mgrid[0:h, 0:w]
    edge = ((x % 4 == 0) | (x % 4 == 3) | (y % 4 == 0) | (y % 4 == 3)) & ~emission.any(axis=2)
    moved = np.abs(plain.astype(np.float64) - frame)[edge] / contrast
    print("the plain filter moves the edge pixels by up to %.3g of the contrast (median %.3g)" % (moved.max(), np.median(moved.max(axis=1))))
    assert moved.max() > 0.1


def test_the_rule_on_its_own_under_the_sanitizers_and_its_digests(tmp_path):
    """tests/denoise_demodulated_check.cpp: wpt_denoise.h without the library or a header of HIP, every buffer of the promised
    size; the library's host entry reproduces the program's digests from the inputs the program leaves"""
    exe = str(tmp_path / "denoise_demodulated_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "denoise_demodulated_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:]
    digests = json.loads(r.stdout.decode())
    assert len(digests) == len(cases.KINDS) * len(cases.SIZES) * 4
    negative = False
    for kind in cases.KINDS:
        for w, h in cases.SIZES:
            raw = open(str(tmp_path / ("%s_%dx%d.bin" % (kind, w, h))), "rb").read()
            assert len(raw) == w * h * (6 * 12 + 4 + 2)
            frame, moments, P, n, albedo, emission = (np.frombuffer(raw, np.float32, w * h * 3, k * w * h * 12).reshape(h, w, 3) for k in range(6))
            m = np.frombuffer(raw, np.int32, w * h, w * h * 72).reshape(h, w)
            n_p = np.frombuffer(raw, np.uint16, w * h, w * h * 76).reshape(h, w)
            negative = negative or bool((emission > frame).any())
            assert w * h < 100 or kind == "sky" or ((albedo == 0).any() and (albedo == FLOOR).any() and (albedo == FLOOR / 2).any())
            for iterations in (0, 1, 3, 8):
                got, var = device.denoise_demodulated_host(frame, moments, n_p, (P, n, m), albedo, emission, _abi.DenoiseParams(iterations=iterations),
                                                           0.0, True)
                assert [cases.digest(got), cases.digest(var)] == digests["%s_%dx%d_i%d" % (kind, w, h, iterations)], (kind, w, h, iterations)
    assert negative                                 # some u is negative: an emitter brighter than its pixel


def test_the_cpp_overload_gives_the_host_forms_bits(tmp_path):
    """tests/denoise_demodulated_cpp_api.cpp: WurblPT::denoise with albedo and emission, with a map and with one sample count"""
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "denoise_demodulated_cpp_api")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "denoise_demodulated_cpp_api.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
    w, h = 20, 11
    i = np.arange(w * h)
    x, y = i % w, i // w
    m = ((x // 4 + y // 3) % 3 - 1).astype(np.int32)
    frame = (((i[:, None] * 7 + np.arange(3) * 3) % 16) / 8.0).astype(np.float32)
    moments = (frame * frame * np.float32(1.5)).astype(np.float32)
    albedo = (((i[:, None] * 5 + np.arange(3) * 11) % 9) / 8.0).astype(np.float32)
    emission = np.where((i % 10 == 3)[:, None], frame * np.float32(0.5), 0).astype(np.float32)
    normals = np.zeros((w * h, 3), np.float32)
    normals[m >= 0, 2] = 1
    positions = np.where((m >= 0)[:, None], np.stack([x / 32.0, y / 32.0, -2.0 - 0.5 * m], axis=1), 0).astype(np.float32)
    shaped = lambda a: a.reshape(h, w, -1)
    guide = (shaped(positions), shaped(normals), m.reshape(h, w))
    a, var = device.denoise_demodulated_host(shaped(frame), shaped(moments), (1 + i % 4).reshape(h, w), guide, shaped(albedo), shaped(emission),
                                             _abi.DenoiseParams(iterations=3), 0.0, True)
    b = device.denoise_demodulated_host(shaped(frame), shaped(moments), 2, guide, shaped(albedo), shaped(emission), None, 0.25)
    assert r.stdout.decode().split() == [cases.digest(a), cases.digest(var), cases.digest(b), "kept"]
    plain = device.denoise_host(shaped(frame), shaped(moments), (1 + i % 4).reshape(h, w), guide, _abi.DenoiseParams(iterations=3))
    assert not np.array_equal(a, plain)


def test_the_example_compiles(tmp_path):
    """examples/denoise_textured.cpp builds as its header says (it needs a device to run: tests/test_gpu_first_hit_colours.py)"""
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "denoise_textured.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib,
                    "-o", str(tmp_path / "denoise_textured")], check=True, timeout=300)
