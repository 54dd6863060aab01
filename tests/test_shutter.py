"""The rolling shutter without a GPU: the rule behind wpt_shutter_row_interval / wpt_shutter_span against its restatement in
numpy float32, what is refused and with which words, the new names in the header, the ctypes table and the library, the C++
side (examples/rolling_shutter.cpp builds; mcptRollingShutter insists on a scene bounded for the whole readout), and the
fixture of tests/test_gpu_shutter.py checked with the CPU restatement alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import shutter_cases as cases
from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
F32 = np.float32
INVALID_ARGUMENT = 1
NAMES = ("wpt_shutter_row_interval", "wpt_shutter_span", "wpt_render_shutter_block_device", "wpt_render_shutter_bands_device",
         "wpt_render_shutter_bands", "wpt_render_shutter_block")


def test_row_intervals_and_span_equal_the_numpy_restatement():
    rng = np.random.default_rng(20261021)
    n = 4000
    t0s = rng.uniform(-10.0, 10.0, n).astype(F32)
    t1s = (t0s + rng.uniform(0.0, 2.0, n).astype(F32)).astype(F32)
    t1s[::7] = t0s[::7]  # instant rows
    row_times = rng.uniform(0.0, 0.02, n).astype(F32)
    row_times[::11] = 0.0
    heights = rng.integers(1, 65536, n)
    heights[:200] = 1
    heights[200:400] = 65535
    for i in range(n):
        h = int(heights[i])
        row = int(rng.integers(0, h))
        for from_top in (False, True):
            sh = host.shutter(row_times[i], from_top)
            assert cases.bits(F32(sh.row_time)) == cases.bits(row_times[i])
            a, b = device.shutter_row_interval(sh, t0s[i], t1s[i], h, row)
            ra, rb = cases.rule(t0s[i], t1s[i], row_times[i], from_top, h, row)
            assert cases.bits(a) == cases.bits(ra) and cases.bits(b) == cases.bits(rb), (i, from_top, h, row, a, b, ra, rb)
            if row_times[i] == 0.0:
                assert (a, b) == (t0s[i], t1s[i])
            first, last = device.shutter_span(sh, t0s[i], t1s[i], h)
            assert cases.bits(first) == cases.bits(t0s[i])
            assert cases.bits(last) == cases.bits(cases.rule(t0s[i], t1s[i], row_times[i], False, h, h - 1)[1])
            # the row read last: the top row of a readout from the bottom, the bottom row of one from the top
            assert cases.bits(last) == cases.bits(device.shutter_row_interval(sh, t0s[i], t1s[i], h, 0 if from_top else h - 1)[1])


@pytest.mark.parametrize("from_top", [False, True])
def test_intervals_are_monotone_in_readout_order(from_top):
    rng = np.random.default_rng(7)
    for h in (1, 2, 24, 257):
        for _ in range(20):
            t0 = F32(rng.uniform(-3.0, 3.0))
            t1 = F32(t0 + F32(rng.uniform(0.0, 1.0)))
            sh = host.shutter(F32(rng.uniform(0.0, 0.1)), from_top)
            rows = [device.shutter_row_interval(sh, t0, t1, h, r) for r in range(h)]
            if from_top:
                rows.reverse()
            assert all(rows[k][0] <= rows[k + 1][0] and rows[k][1] <= rows[k + 1][1] for k in range(h - 1))
            assert all(a <= b for a, b in rows)
            first, last = device.shutter_span(sh, t0, t1, h)
            assert first == rows[0][0] == t0 and last == rows[-1][1] == max(b for _, b in rows)


@pytest.mark.parametrize("case", range(7))
def test_invalid_shutters_are_refused_with_their_message(case):
    name, sh, t0, t1, h, words = cases.bad_shutters()[case]
    L = device.lib()
    a, b = C.c_float(), C.c_float()
    pa, pb = C.cast(C.pointer(a), C.c_void_p), C.cast(C.pointer(b), C.c_void_p)
    for st in (L.wpt_shutter_row_interval(C.byref(sh), t0, t1, h, 0, pa, pb), L.wpt_shutter_span(C.byref(sh), t0, t1, h, pa, pb)):
        assert st == INVALID_ARGUMENT and words in L.wpt_last_error().decode(), (name, st, L.wpt_last_error())
    # the render entry points refuse the same shutters with the same words, before they look at the scene
    p = cases.params(t0, t1)
    for st in (L.wpt_render_shutter_block_device(None, None, C.byref(p), C.byref(sh), 32, h, 3, 0, 32 * h, None, None, None),
               L.wpt_render_shutter_bands_device(None, None, C.byref(p), C.byref(sh), 32, h, 3, 8, 0, 1, None, None, None),
               L.wpt_render_shutter_block(None, None, C.byref(p), C.byref(sh), 32, h, 3, 0, 32 * h, C.c_void_p(1)),
               L.wpt_render_shutter_bands(None, None, C.byref(p), C.byref(sh), 32, h, 3, 8, 0, 1, C.c_void_p(1))):
        assert st == INVALID_ARGUMENT and words in L.wpt_last_error().decode(), (name, st, L.wpt_last_error())


def test_rows_outside_the_frame_and_null_shutters_are_refused():
    L = device.lib()
    sh = host.shutter(0.01)
    a, b = C.c_float(), C.c_float()
    pa, pb = C.cast(C.pointer(a), C.c_void_p), C.cast(C.pointer(b), C.c_void_p)
    for row in (24, 25, 0xffffffff):
        assert L.wpt_shutter_row_interval(C.byref(sh), 0.0, 1.0, 24, row, pa, pb) == INVALID_ARGUMENT
        assert "row lies outside the frame" in L.wpt_last_error().decode()
    for height in (0, 65536):
        assert L.wpt_shutter_span(C.byref(sh), 0.0, 1.0, height, pa, pb) == INVALID_ARGUMENT
        assert "height must lie in 1 .. 65535" in L.wpt_last_error().decode()
    with pytest.raises(RuntimeError, match="row lies outside the frame"):
        device.shutter_row_interval(sh, 0.0, 1.0, 24, 24)
    p = host.default_params()
    assert L.wpt_shutter_span(None, 0.0, 1.0, 24, pa, pb) == INVALID_ARGUMENT
    assert L.wpt_render_shutter_block_device(None, None, C.byref(p), None, 32, 24, 3, 0, 768, None, None, None) == INVALID_ARGUMENT
    assert "shutter is NULL" in L.wpt_last_error().decode()
    assert L.wpt_render_shutter_bands(None, None, C.byref(p), None, 32, 24, 3, 8, 0, 1, C.c_void_p(1)) == INVALID_ARGUMENT
    assert "shutter is NULL" in L.wpt_last_error().decode()


def test_new_names_are_declared_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read(), flags=re.S)
    L = device.lib()
    for name in NAMES:
        assert re.search(r"\bwpt_status\s+%s\s*\(" % name, header), name
        assert name in _abi.FUNCTIONS and name in device.EXPORTS
        assert getattr(L, name).argtypes == _abi.FUNCTIONS[name][1]
    assert re.search(r"typedef struct wpt_shutter \{\s*float row_time;\s*uint32_t from_top;\s*uint32_t reserved\[2\];", header)
    assert _abi.STRUCT_SIZES["wpt_shutter"] == (_abi.Shutter, 16)
    # nothing else takes one: sessions, the other sensors and batches of views keep their parameter lists
    for name, (_, argtypes) in _abi.FUNCTIONS.items():
        assert (C.POINTER(_abi.Shutter) in argtypes) == (name in NAMES), name


def compile_cpp(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def test_example_builds_against_include_alone(tmp_path):
    """examples/rolling_shutter.cpp builds as its header says (its run needs a device: tests/test_gpu_shutter.py)"""
    compile_cpp(tmp_path, os.path.join(ROOT, "examples", "rolling_shutter.cpp"), "rolling_shutter")


UNBOUNDED_PROGRAM = r"""
#include <wurblpt/wurblpt.hpp>
#include <wurblpt/shutter.hpp>
using namespace WurblPT;
int main()
{
    Scene scene;
    const int slide = scene.take(new AnimationKeyframes(0.0f, Transformation(vec3(-1.0f, 0.0f, 0.0f)), 4.0f, Transformation(vec3(1.0f, 0.0f, 0.0f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), scene.take(new MaterialLambertian(vec3(0.7f))), slide));
    const Camera camera(Optics(Projection(radians(50.0f), 1.0f)), Transformation::fromLookAt(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f)));
    RollingShutter shutter;
    shutter.rowTime = 0.125f;
    if (shutter.end(0.0f, 0.5f, 8) != 0.5f + 7 * 0.125f)
        return 3;
    scene.updateBVH(0.0f, 0.5f); /* the exposure interval of one row, not the readout's [0, 1.375] */
    SensorRGB sensor(8, 8);
    mcptRollingShutter(sensor, camera, scene, 1, 0.0f, 0.5f, shutter);
    return 0;
}
"""


def test_mcpt_rolling_shutter_insists_on_a_scene_bounded_for_the_readout(tmp_path):
    """the one way to a silently wrong picture -- moving triangles whose boxes cover [t0, t1] only -- is fatal, and before
    anything asks for a device"""
    src = tmp_path / "unbounded.cpp"
    src.write_text(UNBOUNDED_PROGRAM)
    exe = compile_cpp(tmp_path, str(src), "unbounded")
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == -6, (r.returncode, r.stderr.decode()[-500:])  # abort()
    assert b"Scene::updateBVH(t0, shutter.end(...)) must run before mcptRollingShutter()" in r.stderr
    assert b"no HIP device" not in r.stderr


def test_fixture_of_the_gpu_cases_rolls(oracle):
    """The picture the GPU cases are held to, composed on the CPU alone: row r from the restatement's render with row r's interval,
    for host.animated variant 0, t0 = 0, t1 = 0.25 and row_time = 0.75 / 23 read from the top, the scene bounded for the span.  It
    is finite, equals the global-shutter frame of [t0, t1] in the row read first and differs from it in at least half of the
    other rows: a condition on the input (does this shutter roll visibly at 32 x 24?), which the GPU cases then rely on."""
    t0, t1 = F32(0.0), F32(0.25)
    sh = host.shutter(F32(0.75) / F32(23), from_top=True)
    first, last = device.shutter_span(sh, t0, t1, cases.H)
    assert first == 0.0 and abs(float(last) - 1.0) < 1e-6
    scene = host.animated(cases.W, cases.H, 0, first, last)
    rolling = np.zeros((cases.H, cases.W, 3), dtype=np.float32)
    for r, (a, b) in enumerate(cases.intervals(sh, t0, t1)):
        frame, _ = oracle.render(scene, cases.S, cases.params(a, b), block=(r * cases.W, cases.W))
        rolling[r] = frame[r]
    assert np.isfinite(rolling).all() and rolling.sum() > 0
    plain, _ = oracle.render(scene, cases.S, cases.params(t0, t1))
    top = cases.H - 1
    assert cases.bits_equal(rolling[top], plain[top])
    differing = sum(not cases.bits_equal(rolling[r], plain[r]) for r in range(top))
    assert differing >= (cases.H - 1 + 1) // 2, differing
