"""A batch of views (wpt_render_views*, the batch form of mcpt(), DeviceScene.render_views) without a GPU: bad batches are
refused with WPT_ERR_INVALID_ARGUMENT and a message before a device is needed, the C++ overload builds against include/ and
refuses mismatched sensors before any device work, and the Python look-at helper is wpt_host_lookat's Transformation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
INVALID_ARGUMENT = 1

MISMATCH_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <wurblpt/wurblpt.hpp>
using namespace WurblPT;
int main(int argc, char* argv[])
{
    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.7f)));
    scene.take(new MeshInstance(scene.take(generateQuad()), white));
    scene.updateBVH();
    const Camera camera(Optics(Projection(radians(50.0f), 1.0f)), Transformation::fromLookAt(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f)));
    const std::string c = argc > 1 ? argv[1] : "";
    SensorRGB a(8, 8), b(8, 8), wide(9, 8), tall(8, 9), gateDist(8, 8, 0.5f), gateLen(8, 8, 0.0f, 10.0f, 0.0f, 2.0f);
    std::vector<SensorRGB*> sensors;
    std::vector<Camera> cameras;
    if (c == "empty") {
    } else if (c == "fewer_cameras") {
        sensors = { &a, &b };
        cameras = { camera };
    } else if (c == "fewer_sensors") {
        sensors = { &a };
        cameras = { camera, camera };
    } else if (c == "null_sensor") {
        sensors = { &a, nullptr };
        cameras = { camera, camera };
    } else if (c == "width") {
        sensors = { &a, &wide };
        cameras = { camera, camera };
    } else if (c == "height") {
        sensors = { &a, &tall };
        cameras = { camera, camera };
    } else if (c == "distance_gate") {
        sensors = { &a, &gateDist };
        cameras = { camera, camera };
    } else if (c == "path_length_gate") {
        sensors = { &gateLen, &a };
        cameras = { camera, camera };
    }
    try {
        mcpt(sensors, cameras, scene, 1);
    } catch (const std::invalid_argument& e) {
        printf("refused: %s\n", e.what());
        return 0;
    }
    printf("rendered\n");
    return 0;
}
"""


def compile_cpp(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def test_entry_points_are_exported():
    L = device.lib()
    assert "wpt_render_views_device" in device.EXPORTS and "wpt_render_views" in device.EXPORTS
    getattr(L, "wpt_render_views_device")
    getattr(L, "wpt_render_views")


def _cameras(n, animation=-1):
    cams = (_abi.Camera * max(n, 1))()
    for c in cams:
        c.l, c.r, c.b, c.t = -1.0, 1.0, -1.0, 1.0
        c.rotation[3] = 1.0
        c.scaling[:] = [1.0, 1.0, 1.0]
        c.animation = -1
    cams[max(n, 1) - 1].animation = animation
    return cams


# (what is wrong, cameras, view count, frames pointer, width, height, words the message must hold)
BAD_BATCHES = {
    "no_views": (lambda: _cameras(1), 0, 4096, 16, 16, "view_count"),
    "cameras_null": (lambda: None, 2, 4096, 16, 16, "cameras"),
    "frames_null": (lambda: _cameras(2), 2, None, 16, 16, "frames"),
    "animation_below_minus_one": (lambda: _cameras(3, animation=-2), 3, 4096, 16, 16, "animation"),
    "pixels_overflow_32_bits": (lambda: _cameras(2), 2, 4096, 65535, 65535, "exceeds"),
    "pixels_overflow_the_pool": (lambda: _cameras(3), 3, 4096, 65535, 16385, "exceeds"),
}


@pytest.mark.parametrize("case", list(BAD_BATCHES))
def test_bad_batches_are_refused_before_a_device_is_needed(case):
    """Both entry points refuse each bad batch with WPT_ERR_INVALID_ARGUMENT and say why; the scene is NULL here (there is no
    device to upload one to), so the refusal comes before anything looks at the scene or a device."""
    make, n, frames, w, h, words = BAD_BATCHES[case]
    L = device.lib()
    cams = make()
    p = host.default_params()
    fptr = C.c_void_p(frames) if frames is not None else None
    st = L.wpt_render_views_device(None, cams, n, C.byref(p), w, h, 2, fptr, None, None)
    assert st == INVALID_ARGUMENT, case
    msg = L.wpt_last_error().decode()
    assert words in msg and "views" in msg, msg
    st = L.wpt_render_views(None, cams, n, C.byref(p), w, h, 2, fptr)
    assert st == INVALID_ARGUMENT, case
    assert words in L.wpt_last_error().decode()


def test_largest_batch_is_not_refused_for_its_size():
    """2^31 - 1 pixels are allowed: the next refusal is the NULL scene's"""
    L = device.lib()
    cams = _cameras(1)
    p = host.default_params()
    st = L.wpt_render_views_device(None, cams, 1, C.byref(p), 65535, 32768, 2, C.c_void_p(4096), None, None)
    assert st == INVALID_ARGUMENT and "NULL argument" in L.wpt_last_error().decode()


def test_python_refuses_frames_of_the_wrong_shape():
    import torch
    ds = device.DeviceScene.__new__(device.DeviceScene)
    frames = torch.zeros((2, 4, 4, 3), dtype=torch.float32)
    with pytest.raises(AssertionError):
        ds.render_views_into(frames, [_cameras(1)[0]], 1)          # CPU tensor, and 2 frames for 1 camera


MISMATCHES = ["empty", "fewer_cameras", "fewer_sensors", "null_sensor", "width", "height", "distance_gate", "path_length_gate"]


@pytest.fixture(scope="module")
def mismatch_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("views")
    src = tmp / "mismatch.cpp"
    src.write_text(MISMATCH_PROGRAM)
    return compile_cpp(tmp, str(src), "mismatch")


@pytest.mark.parametrize("case", MISMATCHES)
def test_cpp_batch_refuses_mismatched_sensors_before_device_work(mismatch_exe, case):
    r = subprocess.run([mismatch_exe, case], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    assert out.startswith("refused: mcpt:"), out
    assert b"no HIP device" not in r.stderr and b"Rendering" not in r.stderr


def test_camera_rig_example_builds_and_needs_a_device(tmp_path):
    import torch
    exe = compile_cpp(tmp_path, os.path.join(ROOT, "examples", "camera_rig.cpp"), "camera_rig")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the run is covered by tests/test_gpu_views.py")
    r = subprocess.run([exe, "3", "16", "12", "1", str(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"no HIP device" in r.stderr
    assert not os.path.exists(str(tmp_path / "view-000.png"))       # nothing is faked on the CPU


def test_lookat_helper_is_wpt_host_lookat(golden):
    """host.lookat gives wpt_host_lookat's 35 floats, and camera_looking_at puts the
    first ten -- translation, rotation, scaling -- into a copy of the scene's camera and changes nothing else"""
    fin = golden.f32("lookat_in").reshape(-1, 9)
    L = host.lib()
    for row in fin:
        eye, ctr, up = row[0:3].copy(), row[3:6].copy(), row[6:9].copy()
        direct = np.zeros(35, np.float32)
        L.wpt_host_lookat(C.c_void_p(eye.ctypes.data), C.c_void_p(ctr.ctypes.data), C.c_void_p(up.ctypes.data),
                          C.c_void_p(direct.ctypes.data))
        got = host.lookat(eye, ctr, up)
        assert got.dtype == np.float32 and got.shape == (35,)
        assert np.array_equal(got.view(np.uint32), direct.view(np.uint32))
    sc = host.cornell(16, 12, 1, 2)
    host.set_distortion(sc, 3, k1=-0.25, k2=0.09, k3=-0.015, p1=0.0011, p2=-0.0007)
    before = bytes(sc.camera.contents)
    eye, target, up = (0.3, 1.2, 2.5), (0.0, 0.9, -0.5), (0.0, 1.0, 0.0)
    cam = host.camera_looking_at(sc, eye, target, up)
    T = host.lookat(eye, target, up)
    pose = np.array(list(cam.translation) + list(cam.rotation) + list(cam.scaling), np.float32)
    assert np.array_equal(pose.view(np.uint32), T[0:10].view(np.uint32))
    assert bytes(sc.camera.contents) == before                      # the scene's own camera is untouched
    base = _abi.Camera.from_buffer_copy(before)
    for name, _ in _abi.Camera._fields_:
        if name not in ("translation", "rotation", "scaling"):
            a, b = getattr(cam, name), getattr(base, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, name
