"""LightSpot on the GPU.  The oracle knows no spot light, so every check is made against its render of the diffuse twin: the
same description with each LIGHT_SPOT record retyped LIGHT_DIFFUSE (same v[0], same tex[0]).  A spot's contribution is the
twin's where the ray lies inside the cone and 0 elsewhere, and nothing else about a path changes; so
- a cone of 2 pi (cos of the half angle -1) renders the twin bit for bit, in every kernel and schedule;
- the work counters equal the twin's at any opening angle;
- any cone gives 0 <= spot <= twin value by value (float addition and products with non-negative values are monotone);
- direct light only: pixels whose every (surface point, light point) pair lies inside the cone are the twin's, pixels whose
  every pair lies outside are 0."""
import math
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def lights_to_spots(sc, cos_half):
    """retypes every LIGHT_DIFFUSE record LIGHT_SPOT and gives every LIGHT_SPOT record f[0] = cos_half"""
    changed = 0
    for i in range(sc.d.material_count):
        m = sc.d.materials[i]
        if m.type in (_abi.MAT_LIGHT_DIFFUSE, _abi.MAT_LIGHT_SPOT):
            m.type = _abi.MAT_LIGHT_SPOT
            m.f[0] = cos_half
            changed += 1
    assert changed, "the scene has no light"


def spots_to_twin(sc):
    """the diffuse twin: every LIGHT_SPOT record retyped LIGHT_DIFFUSE, v[0] and tex[0] kept (f[0] is not read there)"""
    for i in range(sc.d.material_count):
        if sc.d.materials[i].type == _abi.MAT_LIGHT_SPOT:
            sc.d.materials[i].type = _abi.MAT_LIGHT_DIFFUSE


def full_circle_scenes():
    return {
        "cornell": (lambda: host.cornell(32, 32, 1, 2), None),
        "spheres": (lambda: host.spheres(48, 40, 0), None),
        "mis_test": (lambda: host.mis_test(48, 32, True), None),
        "texture_probe": (lambda: host.texture_probe(48, 32, 0), None),
        "animated": (lambda: host.animated(48, 32, 8, 0.0, 1.0), (0.0, 1.0)),
        "rgl_scene": (lambda: host.rgl_scene(48, 32, 1), None),
    }


def _params(times=None):
    p = host.default_params()
    if times is not None:
        p.t0, p.t1 = times
    return p


@pytest.mark.parametrize("name", list(full_circle_scenes()))
def test_full_circle_spot_is_the_diffuse_light(dev, oracle, name):
    make, times = full_circle_scenes()[name]
    sc = make()
    p = _params(times)
    lights_to_spots(sc, -1.0)
    ds = dev.DeviceScene(sc)
    frame, _ = ds.render(2, params=p)
    kernel = dev.lib().wpt_kernel_name().decode()
    spots_to_twin(sc)
    ref, _ = oracle.render(sc, 2, params=p)
    assert frame.any()
    assert bits_equal(frame, ref), (name, kernel, int((frame.view(np.uint32) != ref.view(np.uint32)).sum()))


def test_full_circle_block_pool_and_two_passes(dev, oracle):
    # a block of the frame
    sc = host.cornell(48, 40, 1, 2)
    lights_to_spots(sc, -1.0)
    ds = dev.DeviceScene(sc)
    block = (317, 911)
    frame, _ = ds.render(3, block=block)
    spots_to_twin(sc)
    ref, _ = oracle.render(sc, 3, block=block)
    assert bits_equal(frame, ref)
    # the pixel pool: more pixels than lanes in flight
    w, h, s = 1024, 640, 2
    sc = host.cornell(w, h, 1, 2)
    lights_to_spots(sc, -1.0)
    frame, _ = dev.DeviceScene(sc).render(s)
    assert dev.lib().wpt_last_render_passes() == 1
    spots_to_twin(sc)
    rows, block = slice(300, 308), (300 * w, 8 * w)
    ref, _ = oracle.render(sc, s, block=block)
    assert bits_equal(frame[rows], ref[rows])
    # two passes (1536 x 1024, 64 spp)
    w, h, s = 1536, 1024, 8
    sc = host.cornell(w, h, 1, 2)
    lights_to_spots(sc, -1.0)
    frame, _ = dev.DeviceScene(sc).render(s)
    assert dev.lib().wpt_last_render_passes() == 2
    spots_to_twin(sc)
    rows, block = slice(500, 504), (500 * w, 4 * w)
    ref, _ = oracle.render(sc, s, block=block)
    assert bits_equal(frame[rows], ref[rows])


@pytest.mark.parametrize("name,cos_half", [("rgl_scene", -1.0), ("rgl_scene", 0.95), ("stage", -1.0), ("stage", None)])
def test_forced_wavefront_form(dev, oracle, name, cos_half):
    """the wavefront form files spot hits with the lights: the single kernel's frame, and at the full circle the twin's"""
    sc = host.rgl_scene(48, 32, 1) if name == "rgl_scene" else host.spot_scene(48, 32, 1)
    if cos_half is not None:
        lights_to_spots(sc, cos_half)
    ds = dev.DeviceScene(sc)
    single, _ = ds.render(2)
    dev.lib().wpt_set_wavefront(1, 0, 0, 0)
    try:
        frame, _ = ds.render(2)
        assert dev.lib().wpt_kernel_name().decode() == "wf_trace + wf_shade"
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert frame.any() and bits_equal(frame, single)
    if cos_half == -1.0:
        spots_to_twin(sc)
        ref, _ = oracle.render(sc, 2)
        assert bits_equal(frame, ref)


def test_full_circle_transient_bins(dev, oracle):
    sc = host.cornell(32, 32, 1, 2)
    lights_to_spots(sc, -1.0)
    edges = np.array([0.5, 3.0, 4.5, np.inf], np.float32)
    frame, bins = dev.DeviceScene(sc).render_transient(2, edges)
    assert "transient" in dev.lib().wpt_kernel_name().decode()
    spots_to_twin(sc)
    for k in range(len(edges) - 1):
        p = host.default_params()
        p.min_path_len = float(edges[k])
        p.max_path_len = float(np.nextafter(edges[k + 1], np.float32(-np.inf)))
        ref, _ = oracle.render(sc, 2, params=p)
        assert bits_equal(bins[k], ref), k
    ref, _ = oracle.render(sc, 2)
    assert bits_equal(frame, ref)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_work_counters_equal_the_twins_at_any_angle(dev, oracle, variant):
    sc = host.spot_scene(32, 24, variant)
    original = [float(sc.d.materials[i].f[0]) for i in range(sc.d.material_count)]
    spots = [i for i in range(sc.d.material_count) if sc.d.materials[i].type == _abi.MAT_LIGHT_SPOT]
    spots_to_twin(sc)
    ref, ref_counters = oracle.render(sc, 2)
    for cos_half in (None, -1.0, 0.5, 0.9999, 2.0):
        for i in spots:
            sc.d.materials[i].type = _abi.MAT_LIGHT_SPOT
            sc.d.materials[i].f[0] = original[i] if cos_half is None else cos_half
        counted, counters = dev.DeviceScene(sc).render(2, with_counters=True)
        assert counters == ref_counters, (cos_half, counters, ref_counters)
        if cos_half == -1.0:
            assert bits_equal(counted, ref)
        if cos_half == 2.0:                                   # no direction is inside: nothing emits
            assert not counted.any()
        spots_to_twin(sc)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_spot_is_bounded_by_its_twin(dev, oracle, variant):
    """multiple bounces (default parameters): 0 <= spot <= twin for every value, exactly; the cone cuts something"""
    sc = host.spot_scene(48, 40, variant)
    frame, _ = dev.DeviceScene(sc).render(3)
    spots_to_twin(sc)
    twin, _ = oracle.render(sc, 3)
    assert np.isfinite(frame).all() and frame.any()
    assert (frame >= 0).all() and (frame <= twin).all(), int((frame > twin).sum())
    assert (frame < twin).any()


# the Cornell box's ceiling light (wpt_host.cpp buildCornell): y = 1.98, x in [-0.24, 0.23], z in [-0.22, 0.16], normal -y
LIGHT_Y, LIGHT_X, LIGHT_Z = 1.98, (-0.24, 0.23), (-0.22, 0.16)


def classify(pos, nrm, half_angle, margin):
    """pixels (interior, on one plane with their 8 neighbours) whose every (surface point, light point) pair is inside /
    outside the cone of `half_angle` around -y, with `margin` to spare; float64.  The samples of a pixel lie in the convex
    hull of its neighbours' centres, which lies in the ball of radius r around its own centre."""
    pos = pos.astype(np.float64)
    nrm = nrm.astype(np.float64)
    h, w, _ = pos.shape
    inside = np.zeros((h, w), bool)
    outside = np.zeros((h, w), bool)
    corners = np.array([[x, LIGHT_Y, z] for x in LIGHT_X for z in LIGHT_Z])
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            P = pos[y - 1:y + 2, x - 1:x + 2].reshape(9, 3)
            N = nrm[y - 1:y + 2, x - 1:x + 2].reshape(9, 3)
            c = pos[y, x]
            if not (np.abs(N - N[4]).max() < 1e-5 and np.abs(P @ N[4] - c @ N[4]).max() < 1e-5 and np.abs(N[4]).sum() > 0.5):
                continue
            # inside: checked at the hull's corners (the cone of a light point and the cone of a surface point are convex)
            d = P[:, None, :] - corners[None, :, :]                        # surface point - light point
            cosang = -d[..., 1] / np.linalg.norm(d, axis=-1)
            if (cosang >= math.cos(half_angle - margin)).all():
                inside[y, x] = True
                continue
            # outside: a lower bound of the angle over the ball around c and the light rectangle
            r = np.linalg.norm(P - c, axis=1).max()
            if c[1] - r >= LIGHT_Y:
                outside[y, x] = True
                continue
            dx = max(LIGHT_X[0] - c[0], 0.0, c[0] - LIGHT_X[1])
            dz = max(LIGHT_Z[0] - c[2], 0.0, c[2] - LIGHT_Z[1])
            horiz = math.hypot(dx, dz) - r
            drop = LIGHT_Y - (c[1] - r)
            if horiz > 0 and math.atan2(horiz, drop) >= half_angle + margin:
                outside[y, x] = True
    return inside, outside


@pytest.mark.parametrize("opening_degrees", [30.0, 70.0])
def test_cone_geometry_direct_light(dev, oracle, opening_degrees):
    """direct light only (max_path_components = 2, no roulette): inside the cone the twin's pixel bit for bit, outside 0.
    30 degrees is the application's spot; there no pixel the camera sees has the whole light in its cone (the floor under
    the light lies between and behind the boxes), so 70 degrees adds an inside class."""
    w, h, s = 96, 96, 2
    sc = host.spot_scene(w, h, 0)
    half = math.radians(opening_degrees) / 2
    spot = next(i for i in range(sc.d.material_count) if sc.d.materials[i].type == _abi.MAT_LIGHT_SPOT)
    if opening_degrees != 30.0:
        sc.d.materials[spot].f[0] = float(np.cos(np.float32(half)))
    cos_half = float(sc.d.materials[spot].f[0])
    p = host.default_params()
    p.max_path_components = 2
    p.rr_threshold = 0.0
    frame, _ = dev.DeviceScene(sc).render(s, params=p)
    spots_to_twin(sc)
    twin, _ = oracle.render(sc, s, params=p)
    gt = oracle.ground_truth(sc, bits=(1 << 0) | (1 << 1))
    half = math.acos(cos_half)      # the angle the kernel tests against
    inside, outside = classify(gt["world_space_positions"], gt["world_space_geometry_normals"], half, math.radians(1.0))
    assert outside.sum() > 50
    assert (frame[outside] == 0).all(), int((frame[outside] != 0).any(axis=-1).sum())
    assert (twin[outside] > 0).any()                                  # the twin lights some of them
    if opening_degrees == 70.0:
        assert inside.sum() > 50
    assert bits_equal(frame[inside], twin[inside])
    assert (frame <= twin).all() and (frame < twin).any()


def test_multi_device_path_equals_one_device(dev):
    for variant in (0, 1):
        sc = host.spot_scene(64, 48, variant)
        one = host.mcpt(sc, 2, workers=1)
        two = host.mcpt(sc, 2, workers=2)
        assert one.any() and bits_equal(one, two), variant
        frame, _ = dev.DeviceScene(sc).render(2)
        assert bits_equal(one, frame)


# examples/stage_lights.cpp: lamps 0.3 x 0.3 at y = 2.4 pointing down, (centre x, z, opening angle in degrees)
LAMPS = [(-1.5, 0.0, 30.0), (0.0, -0.6, 24.0), (1.5, 0.2, 36.0)]


def test_stage_lights_example_renders(dev, tmp_path):
    exe = str(tmp_path / "stage_lights")
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "stage_lights.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, "320", "180", "4", str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    frame = host.image_load(str(tmp_path / "stage.pfm"))
    pos = host.image_load(str(tmp_path / "stage-positions.pfm")).astype(np.float64)
    assert frame.shape == (180, 320, 3) and pos.shape == frame.shape and np.isfinite(frame).all()
    png = host.image_load(str(tmp_path / "stage.png"))
    assert png.dtype == np.uint8 and png.shape == frame.shape
    on_floor = (np.abs(pos[..., 1]) < 1e-3) & (np.abs(pos[..., 0]) < 2.9) & (np.abs(pos[..., 2]) < 1.9) & (np.abs(pos).sum(axis=-1) > 0)
    dark = on_floor.copy()
    for lx, lz, degrees in LAMPS:
        dist = np.hypot(pos[..., 0] - lx, pos[..., 2] - lz)
        pool = on_floor & (dist < 0.2)
        assert pool.sum() > 10
        lit = frame[pool].max(axis=-1) > 0
        assert lit.mean() > 0.9 and frame[pool].mean() > 1e-3, (lx, lz, lit.mean(), frame[pool].mean())
        # surely outside this lamp's cone: 1 degree past the cone from the lamp's nearest point (half a diagonal from its
        # centre), and the pixel's footprint on the floor (< 0.3 deep at this grazing view) on top
        reach = 2.4 * math.tan(math.radians(degrees / 2 + 1.0)) + 0.15 * math.sqrt(2) + 0.3
        dark &= dist > reach
    assert dark.sum() > 200
    assert (frame[dark] == 0).all(), int((frame[dark] != 0).any(axis=-1).sum())
