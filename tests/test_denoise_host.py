"""The denoiser (wpt_postproc_denoise*, wurblpt_amd/csrc/wpt_denoise.h) without a GPU: the entry points are exported and refuse bad
calls before a device is needed; the host form agrees with a float64 restatement of the formula written here from its description;
with a uniform guide it is the dilated B3 convolution and its variance recursion; a constant stays constant; material, normal and
depth edges hold; wpt_denoise.h stands on its own under the sanitizers and the library's host entry reproduces its digests; the
C++ interface (WurblPT::denoise) gives the host form's bits."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_cases as cases
from wurblpt_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
KY = np.array([0.212671, 0.715160, 0.072169])          # the Y row of the RGB -> XYZ matrix without the factor 100
H = np.array([1, 4, 6, 4, 1]) / 16.0


def test_entry_points_are_exported_and_declared():
    L = device.lib()
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    for name in ("wpt_postproc_denoise", "wpt_postproc_denoise_host", "wpt_postproc_denoise_form"):
        assert name in device.EXPORTS and not re.search(r"\d", name)
        getattr(L, name)
        assert re.search(r"\b%s\(" % name, header)
    assert "} wpt_denoise_params;" in header
    assert "#define WPT_ABI_VERSION 5u" in header and _abi.WPT_ABI_VERSION == 5
    p = _abi.DenoiseParams()
    assert (p.sigma_l, p.normal_log2, p.iterations) == (1.0, 7, 5) and p.sigma_z == np.float32(0.1)
    assert (_abi.DENOISE_MAX_ITERATIONS, _abi.DENOISE_MAX_NORMAL_LOG2) == (8, 16)
    # the form of a step is a matter of the step alone, and steps too wide for a tile in LDS gather
    forms = [device.denoise_form(1 << i) for i in range(9)]
    assert set(forms) <= {"tile", "gather"} and forms[3:] == ["gather"] * 6
    unit = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read()
    assert "wpt_k_denoise" in unit.split()


def _call(host_form, arrays, width, height, params, out, variance):
    L = device.lib()
    ptr = [None if a is None else C.c_void_p(a.ctypes.data) for a in arrays + [out, variance]]
    p = None if params is None else C.byref(params)
    if host_form:
        st = L.wpt_postproc_denoise_host(*ptr[:6], width, height, p, ptr[6], ptr[7])
    else:
        st = L.wpt_postproc_denoise(*ptr[:6], width, height, p, ptr[6], ptr[7], None)
    return st, L.wpt_last_error().decode()


@pytest.mark.parametrize("host_form", [True, False])
def test_bad_calls_are_refused_before_a_device_is_needed(host_form):
    w, h = 6, 4
    c = cases.inputs(w, h)
    good = [c["frame"], c["moments"], c["samples_sqrt"], c["positions"], c["normals"], c["materials"]]
    out = np.zeros((h, w, 3), np.float32)
    var = np.zeros((h, w), np.float32)
    P = _abi.DenoiseParams
    bad = [(good[:k] + [None] + good[k + 1:], w, h, P(), out, var, "input is NULL") for k in range(6)]
    bad += [(good, w, h, P(), None, var, "output frame is NULL")]
    bad += [(good, ww, hh, P(), out, var, "width and height") for ww, hh in ((0, h), (w, 0), (65536, 1), (1, 65536))]
    bad += [(good, w, h, P(iterations=9), out, var, "iterations"), (good, w, h, P(normal_log2=17), out, var, "normal_log2")]
    bad += [(good, w, h, P(sigma_l=s), out, var, "sigma") for s in (0.0, -1.0, math.inf, math.nan)]
    bad += [(good, w, h, P(sigma_z=s), out, var, "sigma") for s in (0.0, -0.1, math.inf, math.nan)]
    # aliasing: an output that is an input, that overlaps one in part, and the two outputs on one another
    bad += [(good, w, h, P(), good[k], var, "aliases") for k in (0, 1, 3, 4)]
    bad += [(good, w, h, P(), out, good[5].view(np.float32), "aliases"), (good, w, h, P(), out, out.reshape(-1)[7:7 + w * h], "aliases")]
    tail = np.zeros(w * h * 3 + 5, np.float32)
    bad += [([tail[5:]] + good[1:], w, h, P(), tail[:w * h * 3], None, "aliases")]
    for arrays, ww, hh, params, o, v, what in bad:
        st, msg = _call(host_form, arrays, ww, hh, params, o, v)
        assert st == INVALID_ARGUMENT and "denoise" in msg and what in msg, (what, st, msg)
    if host_form:   # the good call passes, with the defaults for no parameters and without a variance plane
        assert _call(True, good, w, h, None, out, None)[0] == 0 and _call(True, good, w, h, P(), out, var)[0] == 0
        assert np.isfinite(out).all() and np.isfinite(var).all()


def _shift(a, ox, oy):
    """a[y + oy, x + ox] where that lies inside the frame, and the mask of where it does"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    valid = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        valid[y0:y1, x0:x1] = True
    return out, valid


def reference(frame, moments, n_p, P, n, m, sigma_l=1.0, sigma_z=0.1, normal_log2=7, iterations=5):
    """The filter as its description states it, in float64; returns the frame and the variance plane."""
    f, mo, P, n = (a.astype(np.float64) for a in (frame, moments, P, n))
    N = n_p.astype(np.float64) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where((n_p >= 2)[..., None], np.maximum(mo - f * f, 0) / (N - 1)[..., None], f * f)
    V = (np.sqrt(v) @ KY) ** 2
    c = f
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
    return c, V


def _relative(got, want):
    """the largest |got - want| / |want| (0 where both are 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(got == want, 0, np.abs(got - want) / np.abs(want))
    return float(r.max())


def _seeded_case():
    """24 x 17, seeded: several materials and sky, normals a few degrees around each material's, rough slanted planes, n_p in
    {0, 1, 2, 5}.  Two things keep the comparison of a float filter with a float64 one well conditioned: the second moments stay
    clear of the mean's square on either side (a quarter of it above, or half of it below: clamped), and every 2 x 2 block holds a
    pixel with variance, so no pixel's neighbourhood mean g is exactly 0 -- there L is 1e-10 and a luminance difference of one
    rounding decides whether a tap counts at all.  (That case runs in tests/denoise_check.cpp and, bit for bit, on the GPU.)"""
    w, h = 24, 17
    c = cases.inputs(w, h, "mixed", seed=7)
    rng = np.random.RandomState(77)
    y, x = np.mgrid[0:h, 0:w]
    n_p = np.array([1, 2, 5], np.uint16)[rng.randint(0, 3, (h, w))]
    n_p[(x % 3 == 0) & (y % 3 == 0)] = 0
    frame = (0.25 + rng.rand(h, w, 3) * 4).astype(np.float32)
    frame[n_p == 0] = 0
    clamped = ((x % 3 == 1) & (y % 3 == 1))[..., None]
    moments = (frame * frame * np.where(clamped, 0.5, 1.25 + rng.rand(h, w, 3))).astype(np.float32)
    c.update(frame=frame, moments=moments, samples_sqrt=n_p)
    assert set(np.unique(n_p)) == {0, 1, 2, 5} and (c["materials"] < 0).any() and len(np.unique(c["materials"])) == 5
    return c


@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
def test_host_form_is_the_formula_in_float64(iterations):
    c = _seeded_case()
    got, var = device.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), _abi.DenoiseParams(iterations=iterations), True)
    want, want_var = reference(c["frame"], c["moments"], c["samples_sqrt"], *cases.guide(c), iterations=iterations)
    print("iterations %d: colour %.3g, variance %.3g relative" % (iterations, _relative(got, want), _relative(var, want_var)))
    assert _relative(got, want) <= 1e-4 and _relative(var, want_var) <= 1e-4
    if iterations == 0:
        assert np.array_equal(got, c["frame"])
    else:
        assert not np.array_equal(got, c["frame"])


def _uniform_guide(w, h):
    y, x = np.mgrid[0:h, 0:w]
    P = np.stack([x / 64.0, y / 64.0, np.full((h, w), -3.0)], axis=2).astype(np.float32)
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = 1
    return P, n, np.zeros((h, w), np.int32)


def test_uniform_guide_gives_the_dilated_b3_convolution():
    """one material, one plane, one normal and sigma_l = 1e30: every weight is h[dy] * h[dx], so 62 pixels from the borders the
    result after five iterations is the separable convolution with the B3 kernel dilated by 1, 2, 4, 8, 16, and the variance its
    recursion with the squared weights"""
    w, h = 131, 127
    rng = np.random.RandomState(5)
    frame = (rng.rand(h, w, 3) * 3).astype(np.float32)
    moments = (frame * frame * (1.5 + rng.rand(h, w, 3))).astype(np.float32)
    got, var = device.denoise_host(frame, moments, 2, _uniform_guide(w, h), _abi.DenoiseParams(sigma_l=1e30), True)
    c = frame.astype(np.float64)
    d = moments.astype(np.float64) - c * c
    V = (np.sqrt(d / 3) @ KY) ** 2
    for i in range(5):
        s = 2 ** i
        for axis in (0, 1):
            c = sum(H[k + 2] * np.roll(c, -k * s, axis=axis) for k in range(-2, 3))
        V = sum(H[a + 2] ** 2 * H[b + 2] ** 2 * np.roll(np.roll(V, -a * s, axis=0), -b * s, axis=1) for a in range(-2, 3) for b in range(-2, 3))
    inner = (slice(62, h - 62), slice(62, w - 62))          # further than 62 pixels from a border, np.roll's wrap has not arrived
    assert got[inner].size >= 9 * 3
    assert _relative(got[inner], c[inner]) <= 1e-5 and _relative(var[inner], V[inner]) <= 1e-5


@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
def test_a_constant_colour_stays_constant(iterations):
    c = cases.inputs(33, 20, "mixed", seed=3)
    colour = np.array([0.7, 1.9, 0.3], np.float32)
    frame = np.broadcast_to(colour, c["frame"].shape).copy()
    moments = (frame * frame * 1.5).astype(np.float32)
    got = device.denoise_host(frame, moments, c["samples_sqrt"], cases.guide(c), _abi.DenoiseParams(iterations=iterations))
    assert _relative(got, frame) <= 1e-5 * iterations


def _halves(w, h):
    left = np.array([1.0, 0.5, 0.25], np.float32)
    right = np.array([0.125, 2.0, 1.0], np.float32)
    frame = np.empty((h, w, 3), np.float32)
    frame[:, :w // 2] = left
    frame[:, w // 2:] = right
    moments = (frame * frame * 1.5).astype(np.float32)
    return frame, moments


def test_material_and_normal_edges_hold():
    """two half frames of constant colours with a loud variance estimate (n_p = 1: sigma = value), so that the colour weight
    alone would mix them: apart by material index, then by normals 90 degrees apart (w_n = 0 exactly)"""
    w, h = 40, 12
    frame, moments = _halves(w, h)
    P, n, m = _uniform_guide(w, h)
    by_material = m.copy()
    by_material[:, w // 2:] = 3
    by_normal = n.copy()
    by_normal[:, w // 2:] = (1, 0, 0)
    for guide in ((P, n, by_material), (P, by_normal, m)):
        for iterations in (1, 5, 8):
            got = device.denoise_host(frame, moments, 1, guide, _abi.DenoiseParams(iterations=iterations, sigma_l=1e30, sigma_z=1e30))
            assert _relative(got, frame) <= 1e-5
    # and without either edge the halves do mix
    got = device.denoise_host(frame, moments, 1, (P, n, m), _abi.DenoiseParams(sigma_l=1e30, sigma_z=1e30))
    assert _relative(got, frame) > 0.1


@pytest.mark.parametrize("sigma_z", [0.1, 0.5])
def test_a_depth_edge_leaks_what_the_plane_term_allows(sigma_z):
    """equal normals, the right half one unit behind the left, pixels 1e-4 apart: a tap across the edge leaves the tangent plane
    by an angle whose squared sine is at least s0 = 1 / (1 + (2 * 128 * 1e-4)^2 * 2), so its weight is at most h h exp(-s0 /
    sigma_z^2).  The taps across the edge weigh at most 5/16 of the kernel and the centre 9/64, so an iteration moves a pixel by at
    most 20/9 exp(-s0 / sigma_z^2) of the halves' difference (all colours stay between the halves'), and I iterations by I times
    that; 1e-5 relative on top for the rounding of a constant.  With sigma_z = 0.1 nothing crosses (exp(-100)); with 0.5 the
    leak is there and inside the bound."""
    w, h = 40, 12
    frame, moments = _halves(w, h)
    y, x = np.mgrid[0:h, 0:w]
    P = np.stack([x * 1e-4, y * 1e-4, np.where(x < w // 2, -2.0, -3.0)], axis=2).astype(np.float32)
    _, n, m = _uniform_guide(w, h)
    s0 = 1 / (1 + 2 * (2 * 128 * 1e-4) ** 2)
    for iterations in (1, 5, 8):
        got = device.denoise_host(frame, moments, 1, (P, n, m), _abi.DenoiseParams(iterations=iterations, sigma_l=1e30, sigma_z=sigma_z))
        leak = float((np.abs(got.astype(np.float64) - frame) / np.abs(frame[:, :1].astype(np.float64) - frame[:, -1:])).max())
        bound = iterations * 20 / 9 * math.exp(-s0 / sigma_z ** 2) + 1e-5 * float((frame / np.abs(frame[0, 0] - frame[0, -1])).max())
        print("sigma_z %g, %d iterations: leak %.3g of the difference, bound %.3g" % (sigma_z, iterations, leak, bound))
        assert leak <= bound
        assert sigma_z < 0.5 or leak > 1e-3


def test_the_filter_on_its_own_under_the_sanitizers_and_its_digests(tmp_path):
    """tests/denoise_check.cpp: wpt_denoise.h without the library or a header of HIP, every buffer of the promised size; its digests
    are tests/golden/denoise_digests.json's, and the library's host entry reproduces them from the inputs the program leaves"""
    exe = str(tmp_path / "denoise_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "denoise_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:]
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "denoise_digests.json")))
    assert json.loads(r.stdout.decode()) == golden
    assert len(golden) == len(cases.KINDS) * len(cases.SIZES) * 9
    for kind in cases.KINDS:
        for w, h in cases.SIZES:
            raw = open(str(tmp_path / ("%s_%dx%d.bin" % (kind, w, h))), "rb").read()
            assert len(raw) == w * h * (4 * 12 + 4 + 2)
            frame, moments, P, n = (np.frombuffer(raw, np.float32, w * h * 3, k * w * h * 12).reshape(h, w, 3) for k in range(4))
            m = np.frombuffer(raw, np.int32, w * h, w * h * 48).reshape(h, w)
            n_p = np.frombuffer(raw, np.uint16, w * h, w * h * 52).reshape(h, w)
            assert (kind != "sky" or (m < 0).all()) and (kind != "unsampled" or (n_p == 0).all())
            assert kind != "mixed" or w * h < 100 or ((m < 0).any() and len(np.unique(m)) == 5 and len(np.unique(n_p)) == 4)
            for iterations in range(9):
                got, var = device.denoise_host(frame, moments, n_p, (P, n, m), _abi.DenoiseParams(iterations=iterations), True)
                assert [cases.digest(got), cases.digest(var)] == golden["%s_%dx%d_i%d" % (kind, w, h, iterations)], (kind, w, h, iterations)


def test_the_cpp_interface_gives_the_host_forms_bits(tmp_path):
    """tests/denoise_cpp_api.cpp: WurblPT::denoise with a map and with one sample count, on arrays made again here"""
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "denoise_cpp_api")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "denoise_cpp_api.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
    w, h = 20, 11
    i = np.arange(w * h)
    x, y = i % w, i // w
    m = ((x // 4 + y // 3) % 3 - 1).astype(np.int32)
    frame = (((i[:, None] * 7 + np.arange(3) * 3) % 16) / 8.0).astype(np.float32)
    moments = (frame * frame * np.float32(1.5)).astype(np.float32)
    normals = np.zeros((w * h, 3), np.float32)
    normals[m >= 0, 2] = 1
    positions = np.where((m >= 0)[:, None], np.stack([x / 32.0, y / 32.0, -2.0 - 0.5 * m], axis=1), 0).astype(np.float32)
    shaped = lambda a: a.reshape(h, w, -1)
    guide = (shaped(positions), shaped(normals), m.reshape(h, w))
    a, var = device.denoise_host(shaped(frame), shaped(moments), (1 + i % 4).reshape(h, w), guide, _abi.DenoiseParams(iterations=3), True)
    b = device.denoise_host(shaped(frame), shaped(moments), 2, guide)
    assert r.stdout.decode().split() == [cases.digest(a), cases.digest(var), cases.digest(b), "kept"]
    assert not np.array_equal(a, shaped(frame))
