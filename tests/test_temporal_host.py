"""Temporal accumulation (wpt_postproc_temporal_accumulate*, wpt_postproc_denoise_history*, wurblpt_amd/csrc/wpt_temporal.h) without a
GPU: the layout; a first frame's history is the denoiser's own records and filters to the denoiser's bits; frames at rest
accumulate to their mean and the variance to sum(V) / K^2; whole-pixel motion is exact; fractional and random motion agree with a
float64 restatement of the rule (tests/temporal_cases.py); every way of losing history resets; unsampled pixels carry their history;
bad calls are refused before a device is needed; wpt_temporal.h stands on its own under the sanitizers and the library's host
entry reproduces its digests."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_cases as cases
from tests import temporal_cases as tc
from wurblpt_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
EPS = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def acc(frame, g, motion=None, history=None, params=None):
    """one frame (a dict of temporal_cases.sequence) over the guide g into a history on the host"""
    return device.temporal_accumulate_host(frame["frame"], frame["moments"], frame["samples_sqrt"], cases.guide(g), motion, history, params)


def records(frame, g):
    """prepare()'s records of a frame, as a first-frame history holds them"""
    return acc(frame, g)


def test_entry_points_and_layout():
    L = device.lib()
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    for name in ("wpt_postproc_temporal_accumulate", "wpt_postproc_temporal_accumulate_host", "wpt_postproc_denoise_history",
                 "wpt_postproc_denoise_history_host"):
        assert name in device.EXPORTS
        getattr(L, name)
        assert re.search(r"\b%s\(" % name, header)
    assert "} wpt_temporal_params;" in header and "#define WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL 48u" in header
    assert "#define WPT_ABI_VERSION 5u" in header and _abi.WPT_ABI_VERSION == 5
    assert C.sizeof(_abi.TemporalParams) == 16 == _abi.STRUCT_SIZES["wpt_temporal_params"][1]
    assert _abi.TEMPORAL_HISTORY_BYTES_PER_PIXEL == 48
    p = device.temporal_params()
    assert (p.max_history, p.reserved) == (32.0, 0) and p.normal_cos_min == np.float32(0.9) and p.position_tolerance == np.float32(0.02)
    assert "wpt_k_temporal" in open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read().split()
    g, (f,) = tc.sequence(5, 3, 1)
    assert acc(f, g).nbytes == 5 * 3 * 48


@pytest.mark.parametrize("size", tc.SIZES)
def test_a_first_frame_is_the_denoisers_records(size):
    """history_prev = NULL: the planes are prepare()'s records word for word, with B.w = 1.0f -- and 0.0f in a pixel the frame did
    not sample, as the rule sets it for a pixel without history (denoise_cases' maps hold n_p = 0) -- and the filter on that
    history gives wpt_postproc_denoise_host's bits for 0, 1 and 5 iterations"""
    w, h = size
    c = cases.inputs(w, h, "mixed", seed=2)
    history, length = device.temporal_accumulate_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), length_out=True)
    assert history.shape == (3, h, w, 4) and history.dtype == np.float32
    frame0, V = device.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), _abi.DenoiseParams(iterations=0), True)
    assert np.array_equal(bits(frame0), bits(c["frame"]))
    n = np.where(c["samples_sqrt"] > 0, np.float32(1), np.float32(0)).astype(np.float32)
    want = np.empty((3, h, w, 4), np.float32)
    want[0, ..., :3], want[0, ..., 3] = c["positions"], c["materials"].view(np.float32)
    want[1, ..., :3], want[1, ..., 3] = c["normals"], n
    want[2, ..., :3], want[2, ..., 3] = c["frame"], V
    assert np.array_equal(bits(history), bits(want))
    assert np.array_equal(bits(length), bits(n)) and (w * h < 100 or ((n == 1).any() and (n == 0).any()))
    for iterations in (0, 1, 5):
        p = _abi.DenoiseParams(iterations=iterations)
        got = device.denoise_history_host(history, p, True)
        ref = device.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), p, True)
        assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1])), iterations
    alone = device.denoise_history_host(history)   # the defaults, no variance plane
    assert np.array_equal(bits(alone), bits(device.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c))))
    assert np.array_equal(bits(history), bits(want)), "the filter wrote the history"


@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("size", tc.SIZES)
def test_frames_at_rest_accumulate_to_their_mean(size, K):
    """NULL offsets, K seeded frames over one guide, max_history = 32: N = K everywhere; the colour lies within 4 K 2^-24 max|frame
    values at that pixel and channel| of the float64 mean (four roundings per step, K - 1 steps), the variance within the same
    bound of sum(V_k) / K^2"""
    w, h = size
    g, frames = tc.sequence(w, h, K)
    history = None
    for f in frames:
        history, length = device.temporal_accumulate_host(f["frame"], f["moments"], f["samples_sqrt"], cases.guide(g), history=history, length_out=True)
    assert np.array_equal(history[1, ..., 3], np.full((h, w), K, np.float32)) and np.array_equal(length, history[1, ..., 3])
    stack = np.stack([f["frame"] for f in frames]).astype(np.float64)
    V = np.stack([records(f, g)[2, ..., 3] for f in frames]).astype(np.float64)
    err_c = np.abs(history[2, ..., :3] - stack.mean(axis=0)) / np.abs(stack).max(axis=0)
    err_v = np.abs(history[2, ..., 3] - V.sum(axis=0) / K ** 2) / V.max(axis=0)
    print("K = %d at %dx%d: colour %.3g, variance %.3g of K 2^-24 max" % (K, w, h, err_c.max() / (K * EPS), err_v.max() / (K * EPS)))
    assert err_c.max() <= 4 * K * EPS and err_v.max() <= 4 * K * EPS
    # the guide planes are the current frame's
    assert np.array_equal(bits(history[0]), bits(records(frames[-1], g)[0])) and np.array_equal(bits(history[1, ..., :3]), bits(g["normals"]))


def test_max_history_stops_the_length():
    g, frames = tc.sequence(33, 9, 7)
    history = None
    lengths = []
    for f in frames:
        history = acc(f, g, history=history, params=device.temporal_params(max_history=4))
        lengths.append(float(history[1, ..., 3].max()))
        assert (history[1, ..., 3] == lengths[-1]).all()
    assert lengths == [1, 2, 3, 4, 4, 4, 4]
    # at the stop the newest frame weighs 1 / 4: an exponential mean
    before = acc(frames[5], g, history=acc(frames[4], g, history=None), params=device.temporal_params(max_history=2))
    want = 0.5 * frames[4]["frame"].astype(np.float64) + 0.5 * frames[5]["frame"]
    assert np.abs(before[2, ..., :3] - want).max() <= 4 * EPS * 4.125


@pytest.mark.parametrize("size", tc.SIZES)
def test_whole_pixel_motion_is_exact(size):
    """the previous guide is the current one shifted by (3, -2), with offsets that say so: a pixel whose source lies in the frame
    (and shows a surface: with offsets given, m < 0 resets) equals the rest case on the source pixel's history, bit for bit;
    every other pixel is reset with N = 1"""
    w, h = size
    ox, oy = 3, -2
    g, frames = tc.sequence(w, h, 3)
    previous = acc(frames[1], g, history=acc(frames[0], g))                     # two frames at rest: N = 2
    g2, inside = tc.shifted_guide(g, ox, oy)
    pixel = np.broadcast_to(np.array([ox, oy], np.float32), (h, w, 2)).copy()
    got = acc(frames[2], g2, (pixel, np.zeros((h, w, 3), np.float32)), previous)
    moved = np.stack([tc.shifted(previous[k], ox, oy)[0] for k in range(3)])       # the source pixel's history at the pixel
    rest = acc(frames[2], g2, None, moved)
    reset = records(frames[2], g2)
    keeps = inside & (g2["materials"] >= 0)
    assert np.array_equal(bits(got)[:, keeps], bits(rest)[:, keeps]) and (got[1, ..., 3][keeps] == 3).all()
    assert np.array_equal(bits(got)[:, ~keeps], bits(reset)[:, ~keeps]) and (got[1, ..., 3][~keeps] == 1).all()
    assert w * h < 100 or (keeps.any() and (~inside).any() and (inside & ~keeps).any())


def _against_the_restatement(w, h, kind, params):
    g, frames = tc.sequence(w, h, 3, sampled=False)
    previous = acc(frames[1], g, history=acc(frames[0], g))
    rec = records(frames[2], g)
    pixel, camera = tc.motion(g, kind)
    pixel = tc.settle(previous, rec, frames[2]["samples_sqrt"], pixel, camera, **params)
    got = acc(frames[2], g, (pixel, camera), previous, device.temporal_params(params["max_history"], params["normal_cos_min"], params["tolerance"]))
    want = tc.Restated(previous, rec, frames[2]["samples_sqrt"], pixel, camera, **params)
    return got, want, rec, frames[2]["samples_sqrt"]


@pytest.mark.parametrize("kind", ["fractional", "random"])
@pytest.mark.parametrize("size", tc.SIZES)
def test_fractional_motion_is_the_rule_in_float64(size, kind):
    """the offset (0.37, -1.61), and per-pixel offsets from +-3 with one in sixteen NaN, infinite or far outside, against
    temporal_cases.Restated; no validity decision of these inputs lies within 1e-4 relative of its threshold (asserted).
    Tolerance: 16 * 2^-24 times the largest magnitude among the words that enter an output word.  Roundings on the way to a
    colour word: the tap weight (1), its product with the tap's word (1), three sums of four products (3), the sum of weights
    (3), the quotient (1), N_H's own product, sums and quotient enter through a (counted as 2, a <= 1/2 of N's error), a and b
    (2), two products and the last sum (3): 16; the variance word trades the two products b * b and a * a for N's share."""
    w, h = size
    params = dict(max_history=32.0, normal_cos_min=0.9975, tolerance=0.02)
    got, want, rec, n_p = _against_the_restatement(w, h, kind, params)
    assert want.margin() >= tc.MARGIN
    err_c = np.abs(got[2] - want.C) / np.maximum(want.scale_c, 1e-300)
    err_n = np.abs(got[1, ..., 3] - want.B_w) / want.scale_n
    print("%s %dx%d: colour %.3g, length %.3g of 2^-24 max; %d of %d pixels keep history" % (kind, w, h, err_c.max() / EPS, err_n.max() / EPS,
                                                                                           want.valid.sum(), w * h))
    assert err_c.max() <= 16 * EPS and err_n.max() <= 16 * EPS
    assert np.array_equal(bits(got[0]), bits(rec[0])) and np.array_equal(bits(got[1, ..., :3]), bits(rec[1, ..., :3]))
    lost = ~want.valid
    assert np.array_equal(bits(got[2])[lost], bits(rec[2])[lost])
    if w * h > 1000:   # both outcomes of every decision occur
        assert want.valid.sum() > w * h / 8 and lost.sum() > w * h / 8
        n = got[1, ..., 3][want.valid & (n_p > 0)]
        assert (n >= 1).all() and (n != np.round(n)).any()   # lengths are interpolated like the colours


def _flat(w, h):
    """one material, one plane, one normal, every pixel sampled: nothing loses history by itself"""
    g, frames = tc.sequence(w, h, 2)
    y, x = np.mgrid[0:h, 0:w]
    g["positions"] = np.stack([x / 32.0, y / 32.0, np.full((h, w), -3.0)], axis=2).astype(np.float32)
    g["normals"] = np.broadcast_to(np.array([0, 0, 1], np.float32), (h, w, 3)).copy()
    g["materials"] = np.zeros((h, w), np.int32)
    return g, frames


@pytest.mark.parametrize("way", ["material", "normal", "position", "sky", "outside"])
def test_each_way_of_losing_history(way):
    """one pixel of a flat guide loses its history, one case per way: N = 1 and C' = C there, N = 2 everywhere else"""
    w, h = 6, 4
    px, py = 2, 1
    g, frames = _flat(w, h)
    g2 = {k: v.copy() for k, v in g.items()}
    pixel, camera = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 3), np.float32)
    if way == "material":
        g2["materials"][py, px] = 1
    elif way == "normal":      # cosine 0.8 < 0.9
        g2["normals"][py, px] = (0.6, 0, 0.8)
    elif way == "position":    # 0.2 away; the tolerance is 0.02 * |E| = 0.06
        g2["positions"][py, px, 2] -= 0.2
    elif way == "sky":         # nothing hit, in both frames: with offsets given that resets
        for gg in (g, g2):
            gg["materials"][py, px] = -1
            gg["positions"][py, px] = 0
            gg["normals"][py, px] = 0
    else:
        pixel[py, px] = (-10, 0)
    previous = acc(frames[0], g)
    got = acc(frames[1], g2, (pixel, camera), previous)
    N = got[1, ..., 3]
    want = np.full((h, w), 2, np.float32)
    want[py, px] = 1
    assert np.array_equal(N, want)
    assert np.array_equal(bits(got[2, py, px]), bits(records(frames[1], g2)[2, py, px]))
    # the control: without the cause the pixel keeps its history (for the sky: at rest, where m == m_q is all that is asked)
    control = acc(frames[1], g if way != "sky" else g2, None if way == "sky" else (np.zeros_like(pixel), camera), previous)
    assert (control[1, ..., 3] == 2).all()
    # a normal or a position just inside the threshold keeps it
    if way == "normal":
        g2["normals"][py, px] = (math.sin(math.acos(0.91)), 0, 0.91)
        assert acc(frames[1], g2, (pixel, camera), previous)[1, py, px, 3] == 2
    if way == "position":
        g2["positions"][py, px, 2] = g["positions"][py, px, 2] - 0.05
        assert acc(frames[1], g2, (pixel, camera), previous)[1, py, px, 3] == 2


@pytest.mark.parametrize("moving", [False, True])
def test_unsampled_pixels_carry_their_history(moving):
    """n_p = 0: with history the pixel carries it over with N unchanged; without history it starts at N = 0; the next sampled frame
    then replaces it entirely"""
    w, h = 6, 4
    g, _ = _flat(w, h)
    _, frames = tc.sequence(w, h, 4)
    motion = (np.zeros((h, w, 2), np.float32), np.zeros((h, w, 3), np.float32)) if moving else None
    hole = np.zeros((h, w), bool)
    hole[1, 2] = hole[3, 5] = True
    for f in frames[:1] + frames[2:3]:      # frames 0 and 2 do not sample the two pixels
        f["samples_sqrt"][hole] = 0
        f["frame"][hole] = 0
        f["moments"][hole] = 0
    h0 = acc(frames[0], g, motion)
    assert (h0[1, ..., 3][hole] == 0).all() and (h0[1, ..., 3][~hole] == 1).all()
    assert np.array_equal(bits(h0[2]), bits(records(frames[0], g)[2]))
    h1 = acc(frames[1], g, motion, h0)      # sampled: the pixels of length 0 are replaced entirely
    assert (h1[1, ..., 3][hole] == 1).all() and (h1[1, ..., 3][~hole] == 2).all()
    assert np.array_equal(bits(h1[2])[hole], bits(records(frames[1], g)[2])[hole])
    h2 = acc(frames[2], g, motion, h1)      # not sampled: carried over, word for word
    assert np.array_equal(bits(h2[2])[hole], bits(h1[2])[hole]) and (h2[1, ..., 3][hole] == 1).all() and (h2[1, ..., 3][~hole] == 3).all()
    h3 = acc(frames[3], g, motion, h2)
    assert (h3[1, ..., 3][hole] == 2).all() and (h3[1, ..., 3][~hole] == 4).all()
    want = 0.5 * frames[1]["frame"].astype(np.float64) + 0.5 * frames[3]["frame"]
    assert np.abs(h3[2, ..., :3] - want)[hole].max() <= 4 * 2 * EPS * 4.125


def _call(host_form, arrays, pixel, camera, prev, width, height, params, out, length):
    L = device.lib()
    ptr = [None if a is None else C.c_void_p(a.ctypes.data) for a in list(arrays) + [pixel, camera, prev, out, length]]
    p = None if params is None else C.byref(params)
    if host_form:
        st = L.wpt_postproc_temporal_accumulate_host(*ptr[:9], width, height, p, ptr[9], ptr[10])
    else:
        st = L.wpt_postproc_temporal_accumulate(*ptr[:9], width, height, p, ptr[9], ptr[10], None)
    return st, L.wpt_last_error().decode()


@pytest.mark.parametrize("host_form", [True, False])
def test_bad_calls_are_refused_before_a_device_is_needed(host_form):
    w, h = 6, 4
    c = cases.inputs(w, h)
    good = [c["frame"], c["moments"], c["samples_sqrt"], c["positions"], c["normals"], c["materials"]]
    pixel, camera = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 3), np.float32)
    prev, out = np.zeros((3, h, w, 4), np.float32), np.zeros((3, h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    P = _abi.TemporalParams
    bad = [(good[:k] + [None] + good[k + 1:], pixel, camera, prev, w, h, P(), out, "input is NULL") for k in range(6)]
    bad += [(good, pixel, camera, prev, w, h, P(), None, "history_out is NULL")]
    bad += [(good, pixel, camera, prev, ww, hh, P(), out, "width and height") for ww, hh in ((0, h), (w, 0), (65536, 1), (1, 65536))]
    bad += [(good, pixel, None, prev, w, h, P(), out, "both"), (good, None, camera, prev, w, h, P(), out, "both")]
    bad += [(good, pixel, camera, out, w, h, P(), out, "in place"), (good, None, None, out, w, h, P(), out, "in place")]
    bad += [(good, pixel, camera, prev, w, h, P(max_history=v), out, "max_history") for v in (0.0, 0.5, -1.0, math.inf, math.nan)]
    bad += [(good, pixel, camera, prev, w, h, P(normal_cos_min=v), out, "normal_cos_min") for v in (-1.5, 1.001, math.inf, math.nan)]
    bad += [(good, pixel, camera, prev, w, h, P(position_tolerance=v), out, "position_tolerance") for v in (-0.01, math.inf, math.nan)]
    bad += [(good, pixel, camera, prev, w, h, P(reserved=1), out, "reserved")]
    for arrays, po, co, pr, ww, hh, params, o, what in bad:
        st, msg = _call(host_form, arrays, po, co, pr, ww, hh, params, o, length)
        assert st == INVALID_ARGUMENT and "temporal accumulation" in msg and what in msg, (what, st, msg)
    L = device.lib()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    frame_out, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    D = _abi.DenoiseParams
    for hist, ww, hh, params, o, v, what in [(None, w, h, D(), frame_out, var, "history is NULL"), (prev, w, h, D(), None, var, "output frame is NULL"),
                                             (prev, 0, h, D(), frame_out, var, "width and height"), (prev, w, 65536, D(), frame_out, var, "width and height"),
                                             (prev, w, h, D(iterations=9), frame_out, var, "iterations"), (prev, w, h, D(normal_log2=17), frame_out, var, "normal_log2"),
                                             (prev, w, h, D(sigma_l=0.0), frame_out, var, "sigma"), (prev, w, h, D(sigma_z=math.nan), frame_out, var, "sigma"),
                                             (prev, w, h, D(), prev.reshape(-1)[5:5 + w * h * 3], var, "aliases"),
                                             (prev, w, h, D(), frame_out, prev.reshape(-1)[w * h * 11:], "aliases"),
                                             (prev, w, h, D(), frame_out, frame_out.reshape(-1)[3:3 + w * h], "aliases")]:
        if host_form:
            st = L.wpt_postproc_denoise_history_host(p(hist), ww, hh, C.byref(params), p(o), p(v))
        else:
            st = L.wpt_postproc_denoise_history(p(hist), ww, hh, C.byref(params), p(o), p(v), None)
        msg = L.wpt_last_error().decode()
        assert st == INVALID_ARGUMENT and "denoise" in msg and what in msg, (what, st, msg)
    if host_form:   # the good calls pass: the defaults for no parameters, with and without the optional arrays, the extremes of the ranges
        assert _call(True, good, pixel, camera, prev, w, h, None, out, None)[0] == 0
        assert _call(True, good, None, None, None, w, h, P(1.0, -1.0, 0.0), out, length)[0] == 0
        assert _call(True, good, pixel, camera, None, w, h, P(1e30, 1.0, 1e30), out, length)[0] == 0
        assert L.wpt_postproc_denoise_history_host(p(out), w, h, None, p(frame_out), None) == 0 and np.isfinite(frame_out).all()


def test_the_rule_on_its_own_under_the_sanitizers_and_its_digests(tmp_path):
    """tests/temporal_check.cpp: wpt_temporal.h and wpt_denoise.h without the library or a header of HIP, every buffer of the
    promised size; its digests are tests/golden/temporal_digests.json's, and the library's host entries reproduce them from the
    inputs the program leaves"""
    exe = str(tmp_path / "temporal_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "temporal_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:]
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "temporal_digests.json")))
    assert json.loads(r.stdout.decode()) == golden
    assert len(golden) == len(tc.SIZES) * len(tc.MOTIONS)
    for w, h in tc.SIZES:
        for motion in tc.MOTIONS:
            name = "%s_%dx%d" % (motion, w, h)
            history = None
            digests = []
            for k in range(3):
                raw = open(str(tmp_path / ("%s_f%d.bin" % (name, k))), "rb").read()
                assert len(raw) == w * h * (4 * 12 + 4 + 8 + 12 + 2)
                frame, moments, P, n = (np.frombuffer(raw, np.float32, w * h * 3, j * w * h * 12).reshape(h, w, 3) for j in range(4))
                m = np.frombuffer(raw, np.int32, w * h, w * h * 48).reshape(h, w)
                pixel = np.frombuffer(raw, np.float32, w * h * 2, w * h * 52).reshape(h, w, 2)
                camera = np.frombuffer(raw, np.float32, w * h * 3, w * h * 60).reshape(h, w, 3)
                n_p = np.frombuffer(raw, np.uint16, w * h, w * h * 72).reshape(h, w)
                history, length = device.temporal_accumulate_host(frame, moments, n_p, (P, n, m), None if motion == "none" else (pixel, camera),
                                                                  history, length_out=True)
                assert np.array_equal(bits(length), bits(history[1, ..., 3]))
                digests.append(cases.digest(history))
            out, var = device.denoise_history_host(history, _abi.DenoiseParams(iterations=3), True)
            assert digests + [cases.digest(out), cases.digest(var)] == golden[name], name
            if w * h > 1000 and motion != "none":
                N = history[1, ..., 3]
                assert (N == 1).any() and (N > 1).any(), name
