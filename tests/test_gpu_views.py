"""A batch of views on the GPU: one launch renders V frames of one scene, and frame v is bit for bit the oracle's render of
camera v and the plain GPU render of camera v, for every scene kind of the single kernel, cameras that differ in pose, thin
lens, distortion, surround and stereo mode and animation, frames whose waves straddle views, the pixel pool and scenes where a
plain render takes two passes.  Counters of a batch are the sum of the plain renders' counters."""
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def copy_camera(cam):
    return _abi.Camera.from_buffer_copy(cam)


def _rotate(q, v):
    """quaternion (x, y, z, w) applied to v, in float64 (only used to pick poses)"""
    u, w = np.array(q[0:3], np.float64), float(q[3])
    v = np.array(v, np.float64)
    return v + 2.0 * w * np.cross(u, v) + 2.0 * np.cross(u, np.cross(u, v))


def make_cameras(sc, kinds):
    """cameras for scene `sc`: "scene" is its own camera; the others are moved a little to the side and turned towards a point
    ahead of it ("pose"), and some get a thin lens, OpenCV distortion, a 360 degree surround mode or a stereo distance"""
    base = copy_camera(sc.camera.contents)
    eye = np.array(base.translation, np.float64)
    fwd = _rotate(base.rotation, (0.0, 0.0, -1.0))
    right = _rotate(base.rotation, (1.0, 0.0, 0.0))
    dist = max(1.0, float(np.linalg.norm(eye)))
    cams = []
    for i, kind in enumerate(kinds):
        if kind == "scene":
            cams.append(copy_camera(base))
            continue
        if kind in ("distortion", "surround", "stereo"):
            if kind == "distortion":
                host.set_distortion(sc, 3, k1=-0.25, k2=0.09, k3=-0.015, p1=0.0011, p2=-0.0007)
            else:
                host.set_camera_mode(sc, 2 if kind == "surround" else 0, 0.0 if kind == "surround" else 0.03 * dist)
            shaped = copy_camera(sc.camera.contents)
            sc.camera[0] = base
        else:
            shaped = copy_camera(base)
        e = eye + 0.03 * dist * (i + 1) * right + 0.01 * dist * i * np.array([0.0, 1.0, 0.0])
        posed = host.camera_looking_at(sc, e, eye + dist * fwd, (0.0, 1.0, 0.0))
        for name in ("translation", "rotation", "scaling"):
            setattr(shaped, name, getattr(posed, name))
        shaped.animation = -1
        if kind == "lens":
            shaped.lens_radius = 0.02 * dist
            shaped.focus_dist = dist
        cams.append(shaped)
    return cams


def with_camera(sc, cam, fn):
    """fn() while the scene's camera is `cam` (the oracle and the plain render read it from the host scene)"""
    saved = copy_camera(sc.camera.contents)
    sc.camera[0] = cam
    try:
        return fn()
    finally:
        sc.camera[0] = saved


def check_views(dev, oracle, sc, cams, s, params=None, kernel_words=None, oracle_views=None, counters=True):
    """the batch against the plain GPU render of each camera (and its counters), and against the oracle for `oracle_views`"""
    ds = dev.DeviceScene(sc)
    frames = ds.render_views(s, cams, params=params).cpu().numpy()
    name = dev.lib().wpt_kernel_name().decode()
    assert "views" in name, name
    if kernel_words:
        assert kernel_words in name, name
    assert dev.lib().wpt_last_render_passes() == 1
    assert frames.shape == (len(cams), sc.height, sc.width, 3) and np.isfinite(frames).all()
    plain = [with_camera(sc, c, lambda: ds.render(s, params=params)[0]) for c in cams]
    for v in range(len(cams)):
        nbad = int((frames[v].view(np.uint32) != plain[v].view(np.uint32)).sum())
        assert nbad == 0, "view %d: %d of %d values differ from the plain render" % (v, nbad, frames[v].size)
    for v in (range(len(cams)) if oracle_views is None else oracle_views):
        ref, _ = with_camera(sc, cams[v], lambda: oracle.render(sc, s, params=params))
        nbad = int((frames[v].view(np.uint32) != ref.view(np.uint32)).sum())
        assert nbad == 0, "view %d: %d of %d values differ from the oracle" % (v, nbad, frames[v].size)
    if counters:
        counted, cnt = ds.render_views(s, cams, params=params, with_counters=True)
        assert "counting" in dev.lib().wpt_kernel_name().decode()
        counted = counted.cpu().numpy()
        total = None
        for v, c in enumerate(cams):
            f, one = with_camera(sc, c, lambda: ds.render(s, params=params, with_counters=True))
            assert bits_equal(counted[v], f), "view %d of the counting batch" % v
            total = one if total is None else {k: total[k] + one[k] for k in total}
        assert cnt == total, (cnt, total)
    return frames


def _hbm_basic():
    return host.cornell(37, 23, 1, 2)


SCENES = {
    # name: (scene, camera kinds, params t0 t1, launch variant, words of the kernel name)
    "cornell_lds": (lambda: host.cornell(37, 23, 1, 2), ["scene", "pose", "pose", "pose"], None, 0, "scene in LDS"),
    "cornell_lds_tiled": (lambda: host.cornell(40, 24, 1, 2), ["pose", "scene", "pose"], None, 0, "scene in LDS"),
    "cornell_one_view": (lambda: host.cornell(37, 23, 1, 2), ["pose"], None, 0, "scene in LDS"),
    "basic_hbm": (_hbm_basic, ["scene", "pose", "pose"], None, 0x01, "views, basic"),
    "cornell_cameras": (lambda: host.cornell(37, 23, 1, 2), ["scene", "lens", "distortion", "surround", "stereo"], None, 0,
                        "all features"),
    "sponza_like": (lambda: host.sponza_like(37, 23, detail=0.05, tex_size=32, env_width=64, importance_n=16),
                    ["scene", "pose", "lens", "distortion", "stereo"], None, 0, "all features"),
    "spheres": (lambda: host.spheres(37, 23, 1), ["scene", "pose", "lens", "surround"], None, 0, "all features"),
    "spot_scene": (lambda: host.spot_scene(37, 23, 0), ["scene", "pose", "distortion"], None, 0, "all features"),
    "animated": (lambda: host.animated(37, 23, 8, 0.0, 1.0), ["scene", "pose", "lens"], (0.0, 1.0), 0, "moving scenes"),
    "rgl_scene": (lambda: host.rgl_scene(37, 23, 1), ["scene", "pose", "lens"], None, 0, "measured BRDFs"),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_views_equal_oracle_and_plain_renders(dev, oracle, name):
    make, kinds, times, variant, words = SCENES[name]
    sc = make()
    if sc.d.envmap.N > 0 and not sc.d.envmap.M:
        sc.set_envmap_tables(*oracle.envmap_tables(sc))     # the oracle takes the importance tables from its caller
    p = host.default_params()
    if times is not None:
        p.t0, p.t1 = times
    cams = make_cameras(sc, kinds)
    if name == "animated":
        assert cams[0].animation >= 0 and cams[1].animation == -1    # an animated camera next to static ones
    dev.lib().wpt_set_launch_config(0, variant)
    try:
        # the oracle has no spot light: spot_scene is held to the plain render here, and to the oracle's diffuse twin below
        frames = check_views(dev, oracle, sc, cams, 2, params=p, kernel_words=words,
                             oracle_views=[] if name == "spot_scene" else None)
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    for v in range(1, len(cams)):
        assert not bits_equal(frames[v], frames[0]), "view %d is the same picture as view 0" % v


def test_spot_views_with_full_circle_cones_equal_the_oracle_twin(dev, oracle):
    """A spot whose cone is the full circle (cos of half the angle -1) emits like LightDiffuse: each view of the batch equals the
    oracle's render of the scene with the spots retyped diffuse"""
    sc = host.spot_scene(37, 23, 0)
    spots = [i for i in range(sc.d.material_count) if sc.d.materials[i].type == _abi.MAT_LIGHT_SPOT]
    assert spots
    for i in spots:
        sc.d.materials[i].f[0] = -1.0
    cams = make_cameras(sc, ["scene", "pose", "lens", "distortion"])
    frames = dev.DeviceScene(sc).render_views(2, cams).cpu().numpy()
    for i in spots:
        sc.d.materials[i].type = _abi.MAT_LIGHT_DIFFUSE
    for v, c in enumerate(cams):
        ref, _ = with_camera(sc, c, lambda: oracle.render(sc, 2))
        assert frames[v].any() and bits_equal(frames[v], ref), "view %d" % v


def turntable(sc, n, radius_scale=1.0):
    """n cameras on a circle around the point the scene's camera looks at (at its distance), all aimed at that point"""
    base = sc.camera.contents
    eye = np.array(base.translation, np.float64)
    fwd = _rotate(base.rotation, (0.0, 0.0, -1.0))
    dist = float(np.linalg.norm(eye))
    centre = eye + dist * fwd
    cams = []
    for i in range(n):
        a = np.radians(-40.0 + 80.0 * i / max(n - 1, 1))
        off = (eye - centre) * radius_scale
        e = centre + np.array([off[0] * np.cos(a) + off[2] * np.sin(a), off[1], -off[0] * np.sin(a) + off[2] * np.cos(a)])
        cams.append(host.camera_looking_at(sc, e, centre, (0.0, 1.0, 0.0)))
    return cams


def test_views_share_waves_and_the_pixel_pool(dev, oracle):
    """37 x 23 frames: waves straddle views at every view boundary; 400 of them are more pixels than the lanes in flight, so
    lanes take pixels from the pool one by one, from any view.  Scene in LDS and the all-features kernel."""
    sc = host.cornell(37, 23, 1, 2)
    cams = turntable(sc, 400)
    s = 1
    for variant, words in ((0, "scene in LDS"), (0x02, "all features")):
        dev.lib().wpt_set_launch_config(0, variant)
        try:
            ds = dev.DeviceScene(sc)
            frames = ds.render_views(s, cams).cpu().numpy()
            assert words in dev.lib().wpt_kernel_name().decode()
            plain = [with_camera(sc, c, lambda: ds.render(s)[0]) for c in cams]
        finally:
            dev.lib().wpt_set_launch_config(0, 0)
        for v in range(len(cams)):
            assert bits_equal(frames[v], plain[v]), "variant %#x view %d" % (variant, v)
    for v in (0, 211, 399):
        ref, _ = with_camera(sc, cams[v], lambda: oracle.render(sc, s))
        assert bits_equal(frames[v], ref), "view %d against the oracle" % v


def test_two_pass_regime(dev, oracle):
    """A scene from HBM at 64 spp with 2 pixels per lane in flight: the plain render takes two passes, the batch one; the
    frames are the same"""
    w, h, s = 1024, 512, 8
    sc = host.cornell(w, h, 1, 2)
    cams = make_cameras(sc, ["scene", "pose", "pose"])
    dev.lib().wpt_set_launch_config(0, 0x01)
    try:
        ds = dev.DeviceScene(sc)
        frames = ds.render_views(s, cams).cpu().numpy()
        assert "views, basic" in dev.lib().wpt_kernel_name().decode()
        assert dev.lib().wpt_last_render_passes() == 1
        for v, c in enumerate(cams):
            plain = with_camera(sc, c, lambda: ds.render(s)[0])
            assert dev.lib().wpt_last_render_passes() == 2
            assert bits_equal(frames[v], plain), "view %d" % v
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    rows = slice(200, 202)
    ref, _ = with_camera(sc, cams[1], lambda: oracle.render(sc, s, block=(200 * w, 2 * w)))
    assert bits_equal(frames[1][rows], ref[rows])


def test_render_views_writes_only_its_own_tensor(dev):
    import torch
    sc = host.cornell(37, 23, 1, 2)
    cams = make_cameras(sc, ["scene", "pose", "pose"])
    ds = dev.DeviceScene(sc)
    out = ds.render_views(2, cams)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (3, 23, 37, 3) and out.dtype == torch.float32
    sentinel = float(np.frombuffer(np.uint32(0x7fc0beef).tobytes(), np.float32)[0])
    big = torch.full((5, 23, 37, 3), sentinel, dtype=torch.float32, device="cuda")
    frames = big[1:4]
    assert frames.is_contiguous()
    ds.render_views_into(frames, cams, 2, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    got = big.cpu().numpy()
    for k in (0, 4):
        assert (got[k].view(np.uint32) == 0x7fc0beef).all(), "frame %d outside the batch was written" % k
    assert bits_equal(got[1:4], out.cpu().numpy())


def test_camera_animation_outside_the_scene_is_refused(dev):
    sc = host.cornell(16, 16, 1, 2)
    cams = make_cameras(sc, ["scene", "pose"])
    cams[1].animation = 0                                     # the Cornell box has no animations
    ds = dev.DeviceScene(sc)
    with pytest.raises(RuntimeError, match="camera 1 refers to an animation outside"):
        ds.render_views(1, cams)


CPP_BATCH = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <wurblpt/wurblpt.hpp>
using namespace WurblPT;
int main()
{
    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.7f)));
    Material* metal = scene.take(new MaterialGGX(vec3(1.0f), vec2(0.1f)));
    Material* light = scene.take(new LightDiffuse(vec3(6.0f)));
    scene.take(new MeshInstance(scene.take(generateQuad()), white, Transformation(vec3(0.0f), toQuat(radians(-90.0f), vec3(1.0f, 0.0f, 0.0f)), vec3(3.0f))));
    scene.take(new MeshInstance(scene.take(generateCube()), metal, Transformation(vec3(0.0f, 0.5f, 0.0f), quat::null(), vec3(0.5f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), light, Transformation(vec3(0.0f, 2.5f, 0.0f), toQuat(radians(90.0f), vec3(1.0f, 0.0f, 0.0f)), vec3(0.5f))), HotSpot);
    scene.updateBVH();
    const unsigned int w = 29, h = 19, views = 4;
    std::vector<Camera> cameras;
    for (unsigned int v = 0; v < views; v++) {
        const float a = radians(30.0f * v);
        Camera c(Optics(Projection(radians(50.0f), float(w) / h)), Transformation::fromLookAt(vec3(4.0f * std::sin(a), 2.0f, 4.0f * std::cos(a)), vec3(0.0f, 0.5f, 0.0f)));
        if (v == 2)
            c.optics.depthOfField = LensDepthOfField(0.1f, 4.0f);
        cameras.push_back(c);
    }
    std::vector<SensorRGB> store;
    store.reserve(views);
    std::vector<SensorRGB*> sensors;
    for (unsigned int v = 0; v < views; v++) {
        store.emplace_back(w, h);
        sensors.push_back(&store.back());
    }
    mcpt(sensors, cameras, scene, 3);
    int bad = 0;
    for (unsigned int v = 0; v < views; v++) {
        SensorRGB single(w, h);
        mcpt(single, cameras[v], scene, 3);
        if (memcmp(single.result().data(), sensors[v]->result().data(), size_t(w) * h * 3 * sizeof(float)) != 0) {
            printf("view %u differs\n", v);
            bad++;
        }
        for (const char* tag : { "WURBLPT/SAMPLES_PER_PIXEL", "WURBLPT/MAX_PATH_COMPONENTS", "WURBLPT/RUSSIAN_ROULETTE_THRESHOLD",
                                 "WURBLPT/COMPILER", "WURBLPT/DEVICE_MODEL", "WURBLPT/DEVICE_COUNT" })
            if (single.result().globalTagList().value(tag) != sensors[v]->result().globalTagList().value(tag)) {
                printf("tag %s differs\n", tag);
                bad++;
            }
        if (sensors[v]->result().globalTagList().value("WURBLPT/DEVICE_KERNEL").find("views") == std::string::npos) {
            printf("kernel tag\n");
            bad++;
        }
    }
    printf(bad ? "FAIL\n" : "OK\n");
    return bad ? 1 : 0;
}
"""


def compile_cpp(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def test_cpp_batch_sensors_equal_single_mcpt(tmp_path):
    src = tmp_path / "batch.cpp"
    src.write_text(CPP_BATCH)
    exe = compile_cpp(tmp_path, str(src), "batch")
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("OK"), (r.stdout.decode(), r.stderr.decode()[-2000:])


def test_camera_rig_example_runs(tmp_path):
    exe = compile_cpp(tmp_path, os.path.join(ROOT, "examples", "camera_rig.cpp"), "camera_rig")
    r = subprocess.run([exe, "5", "40", "30", "2", str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"5 views" in r.stdout and b"views" in r.stdout.split(b"kernel")[-1]
    for v in range(5):
        assert os.path.getsize(str(tmp_path / ("view-%03u.png" % v))) > 0
