"""The time-of-flight sensor on the GPU.  The oracle has no ToF, so exactness is pinned by identities against what exists:
a twin scene whose LightSpot puts into the x channel what the ToF light puts into the fourth (rendered with SensorRGB), the
one-phase launch for every plane of a several-phase launch, every schedule and kernel form against each other, geometry for
the decoded phase, and a slab whose near infrared index differs for the fourth channel of the optical path length."""
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32
C_LIGHT = 299792458.0


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def params(max_path_components=None, jitter=True, times=None, rr=None):
    p = host.default_params()
    if max_path_components is not None:
        p.max_path_components = max_path_components
    p.randomize_ray_over_pixel = 1 if jitter else 0
    if rr is not None:
        p.rr_threshold = rr
    if times is not None:
        p.t0, p.t1 = times
    return p


class kernel_choice:
    """variant word of wpt_set_launch_config for the duration of a block (0 = the library's choice, 0x02 = all features,
    0x10 = no pixel pool, 0x40 = never two passes), as tests/test_gpu_transient.py switches"""

    def __init__(self, dev, variant):
        self.dev, self.variant = dev, variant

    def __enter__(self):
        self.dev.lib().wpt_set_launch_config(0, self.variant)

    def __exit__(self, *a):
        self.dev.lib().wpt_set_launch_config(0, 0)


def kernel_name(dev):
    return dev.lib().wpt_kernel_name().decode()


def materials(sc):
    return [sc.d.materials[i] for i in range(sc.d.material_count)]


def x_equals_w(sc):
    """every material that is no light attenuates the x and the fourth channel alike: its colour vectors are given with a
    fourth component equal to the first (decided from the records, before anything is rendered)"""
    for m in materials(sc):
        if m.type in (_abi.MAT_LIGHT_SPOT, _abi.MAT_LIGHT_DIFFUSE, _abi.MAT_TWOSIDED, _abi.MAT_NONE):
            continue
        if m.tex[0] >= 0 or m.normal_tex >= 0:
            return False
        if m.type == _abi.MAT_GLASS:
            vectors = [m.v[0]]                  # the absorption; the index does not attenuate
        elif m.type == _abi.MAT_MODPHONG:
            vectors = [m.v[0], m.v[1], m.v[2], m.v[3]]
            if not (m.flags & 1):
                return False                    # the fourth channel is an average computed on the device
        else:
            vectors = [m.v[0]]
            if not (m.flags & 1):
                return False
        if any(F32(v[0]) != F32(v[3]) for v in vectors):
            return False
    return True


TIMES = {1: (0.5, 0.501)}


def scene_pair(variant, w, h, twin):
    t = TIMES.get(variant, (0.0, 0.0))
    return host.tof_scene(w, h, variant, 0, *t), host.tof_scene(w, h, variant, twin, *t), (t if variant == 1 else None)


def lds_possible(sc):
    feats = {m.type for m in materials(sc)}
    return feats <= {_abi.MAT_LAMBERTIAN, _abi.MAT_GGX, _abi.MAT_GLASS, _abi.MAT_MIRROR, _abi.MAT_LIGHT_DIFFUSE, _abi.MAT_LIGHT_SPOT,
                     _abi.MAT_TWOSIDED} and sc.d.node_count * 32 + sc.d.tri_count * 48 <= 20 * 1024 and sc.d.animation_count == 0


def kernel_variants(sc):
    return (0, 0x02) if lds_possible(sc) else (0x02,)


def test_eligible_twins_are_what_the_scenes_say():
    """which variants have equal x and w albedo: the wall-and-box scene, the slab, the wall alone; the room has ModPhong
    materials given by three channels, whose fourth is their average"""
    assert [v for v in range(5) if x_equals_w(host.tof_scene(16, 16, v, 0, *TIMES.get(v, (0.0, 0.0))))] == [2, 3, 4]


@pytest.mark.parametrize("variant,mpc", [(2, 2), (3, 2), (4, 2), (3, 4)])
def test_twin_exact(dev, variant, mpc):
    """One sample, no jitter: a pixel has at most one non-zero contribution (with two path components the light ray of the
    first hit or nothing; through the slab with four, where glass sends no light rays, the light's own emission at the path's
    end or nothing).  The twin's x value IS that contribution, so `total` is the rule applied to it once, bit for bit."""
    w, h = 48, 40
    sc, twin, _ = scene_pair(variant, w, h, 1)
    assert x_equals_w(sc)
    p = params(mpc, jitter=False)
    for contrast in (0.75, 0.0):
        sensor = host.tof_sensor(contrast=contrast)
        for kv in kernel_variants(sc):
            with kernel_choice(dev, kv):
                planes = dev.DeviceScene(sc).render_tof(1, sensor, params=p)
                name = kernel_name(dev)
                rgb, _ = dev.DeviceScene(twin).render(1, params=p)
            assert "time of flight" in name and ("scene in LDS" in name) == (kv == 0), name
            x = rgb[:, :, 0]
            want = np.zeros((h, w), np.float32)
            for iy in range(h):
                for ix in range(w):
                    want[iy, ix] = dev.tof_accumulate_host(sensor, 0, float(x[iy, ix]), 0.0, 0, np.zeros(3, np.float32))[2]
            # the twin must show light for the identity to say anything.  Behind the slab only the light's own face is lit:
            # a square of side 1 at distance 3 in a frame that spans 4.2 x 5.04 there, 4.7 % of the pixels (with two path
            # components nothing gets through the slab and the identity holds between black frames)
            least = 0 if (variant == 3 and mpc == 2) else (w * h // 40 if variant == 3 else w * h // 8)
            assert (x > 0).sum() >= least, "the twin is dark"
            for j in range(4):
                assert bits_equal(planes[j, :, :, 2], want), (variant, kv, j)
                if contrast == 0.0:
                    assert bits_equal(planes[j, :, :, 0], planes[j, :, :, 1])
                    assert bits_equal(planes[j, :, :, 0], F32(0.5) * planes[j, :, :, 2])
            if contrast > 0 and (x > 0).any():
                lit = x > 0
                assert (planes[0, :, :, 0][lit] != planes[0, :, :, 1][lit]).any()      # the ToF light's share is modulated
                assert np.allclose(planes[:, :, :, 0] + planes[:, :, :, 1], planes[:, :, :, 2], rtol=1e-6)


@pytest.mark.parametrize("variant", [2, 3, 4])
def test_twin_many_samples(dev, variant):
    """64 spp, 6 path components: total = 1000 * pixelArea * 0.5 * exposureTime times the twin's x within (n + 4) * 2^-24
    relative, n = samples * 2 * path components, the most additions a pixel can have; a == b == total / 2 exactly at contrast 0"""
    w, h, s, mpc = 48, 40, 8, 6
    sc, twin, _ = scene_pair(variant, w, h, 1)
    p = params(mpc)
    sensor = host.tof_sensor(contrast=0.0)
    n = s * s * 2 * mpc
    for kv in kernel_variants(sc):
        with kernel_choice(dev, kv):
            planes = dev.DeviceScene(sc).render_tof(s, sensor, phases=[1], params=p)
            rgb, _ = dev.DeviceScene(twin).render(s, params=p)
        total = planes[0, :, :, 2].astype(np.float64)
        want = 1000.0 * 144.0 * 0.5 * 1000.0 * rgb[:, :, 0].astype(np.float64)
        err = np.abs(total - want)
        print("variant %d kernel word %#x: max relative deviation %.3g of %.3g allowed" % (
            variant, kv, (err[want > 0] / want[want > 0]).max(), (n + 4) * U))
        assert (want > 0).sum() > (w * h // 40 if variant == 3 else w * h // 4)      # behind the slab: the light's face, 4.7 % of the frame
        assert (err <= (n + 4) * U * want).all()
        assert bits_equal(planes[0, :, :, 0], planes[0, :, :, 1]) and bits_equal(planes[0, :, :, 0], F32(0.5) * planes[0, :, :, 2])


def test_a_diffuse_light_is_not_modulated(dev):
    """a scene lit by a LightDiffuse only: nothing is from a ToF light, so a == b exactly at contrast 0.75"""
    sc = host.cornell(32, 32, 1, 2)
    sensor = host.tof_sensor(contrast=0.75)
    for kv in (0, 0x02):
        with kernel_choice(dev, kv):
            planes = dev.DeviceScene(sc).render_tof(4, sensor)
        assert planes[:, :, :, 2].min() >= 0 and (planes[0, :, :, 2] > 0).sum() > 512
        assert bits_equal(planes[:, :, :, 0], planes[:, :, :, 1])
        assert bits_equal(planes[:, :, :, 0], F32(0.5) * planes[:, :, :, 2])


@pytest.mark.parametrize("variant,count", [(0, 4), (2, 4), (1, 4), (2, 8), (1, 8), (3, 4)])
def test_phases_in_one_launch(dev, variant, count):
    """plane j of one launch is the one-phase launch with tau_j bit for bit (static scenes and a moving one over the same
    exposure interval), and `total` is the same in every plane"""
    w, h, s = 40, 32, 3
    sc, _, times = scene_pair(variant, w, h, 1)
    p = params(5, times=times)
    sensor = host.tof_sensor(phase_image_count=count, modulation_frequency=20e6)
    for kv in kernel_variants(sc):
        with kernel_choice(dev, kv):
            ds = dev.DeviceScene(sc)
            planes = ds.render_tof(s, sensor, params=p)
            name = kernel_name(dev)
            assert "time of flight" in name and ("moving" in name) == (variant == 1)
            assert planes.shape == (count, h, w, 3) and np.isfinite(planes).all() and (planes[0, :, :, 2] > 0).any()
            for j in range(count):
                one = ds.render_tof(s, sensor, phases=[j], params=p)
                assert bits_equal(one[0], planes[j]), (variant, kv, j)
                assert bits_equal(planes[j, :, :, 2], planes[0, :, :, 2])
            # the phases differ where the ToF light is seen
            assert not bits_equal(planes[0, :, :, 0], planes[count // 2, :, :, 0])
            # any subset, in any order
            sub = ds.render_tof(s, sensor, phases=[count - 1, 1], params=p)
            assert bits_equal(sub[0], planes[count - 1]) and bits_equal(sub[1], planes[1])


def test_block_semantics(dev):
    import torch
    w, h, s = 32, 32, 2
    sc = host.tof_scene(w, h, 2)
    sensor = host.tof_sensor()
    p = params(4)
    ds = dev.DeviceScene(sc)
    whole = ds.render_tof(s, sensor, params=p)
    whole1 = ds.render_tof(s, sensor, phases=[2], params=p)
    sentinel = -7.25
    for phases, ref in ((None, whole), ([2], whole1)):
        n = ref.shape[0]
        planes = torch.full((n, h, w, 3), sentinel, dtype=torch.float32, device="cuda")
        start, size = 100, 333
        ds.render_tof_into(planes, s, sensor, phases, block=(start, size), params=p, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        ds.check()
        got = planes.cpu().numpy().reshape(n, -1, 3)
        inside = np.zeros(w * h, bool)
        inside[start:start + size] = True
        assert (got[:, ~inside] == sentinel).all()
        assert bits_equal(got[:, inside], ref.reshape(n, -1, 3)[:, inside])
        # blocks that tile the frame are one whole-frame launch
        planes.fill_(sentinel)
        for blk in ((0, 517), (517, w * h - 517)):
            ds.render_tof_into(planes, s, sensor, phases, block=blk, params=p, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert bits_equal(planes.cpu().numpy(), ref)
        # the synchronous host form gives the block's values
        hb = ds.render_tof_host(s, sensor, (start, size), phases=phases, params=p)
        assert bits_equal(hb, ref.reshape(n, -1, 3)[:, start:start + size])


def test_kernel_forms_give_the_same_bits(dev):
    """the kernel with the scene in LDS against the all-features kernel, and a forced wavefront setting (the time-of-flight
    launch stays with the single kernel)"""
    w, h, s = 64, 48, 3
    sc = host.tof_scene(w, h, 2)
    sensor = host.tof_sensor()
    p = params(6)
    ds = dev.DeviceScene(sc)
    ref = ds.render_tof(s, sensor, params=p)
    assert "scene in LDS" in kernel_name(dev)
    with kernel_choice(dev, 0x02):
        full = ds.render_tof(s, sensor, params=p)
        assert "all features" in kernel_name(dev)
    assert bits_equal(ref, full)
    dev.lib().wpt_set_wavefront(1, 0, 0, 0)
    try:
        ds.render(s, params=p)
        assert kernel_name(dev) == "wf_trace + wf_shade"
        forced = ds.render_tof(s, sensor, params=p)
        assert "time of flight" in kernel_name(dev)
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert bits_equal(ref, forced)


def test_pool_and_two_pass_schedules(dev):
    """frames larger than the lanes in flight: the pixel pool on and off (scene in LDS and all-features kernel), two passes on
    and off (scene from HBM, 64 spp), one phase and four"""
    sensor = host.tof_sensor()
    p = params(4)
    w, h, s = 1024, 640, 2
    sc = host.tof_scene(w, h, 2)
    for phases in (None, [3]):
        ref = None
        for kv in (0, 0x10, 0x02, 0x02 | 0x10):
            with kernel_choice(dev, kv):
                got = dev.DeviceScene(sc).render_tof(s, sensor, phases=phases, params=p)
                assert dev.lib().wpt_last_render_passes() == 1
            assert (got[0, :, :, 2] > 0).sum() > w * h // 2
            ref = got if ref is None else ref
            assert bits_equal(ref, got), hex(kv)
    s = 8
    for variant, times in ((0, None), (1, TIMES[1])):
        sc = host.tof_scene(w, h, variant, 0, *(times or (0.0, 0.0)))
        pp = params(3, times=times)
        for phases in (None, [1]):
            with kernel_choice(dev, 0x02):
                two = dev.DeviceScene(sc).render_tof(s, sensor, phases=phases, params=pp)
                assert dev.lib().wpt_last_render_passes() == 2
            with kernel_choice(dev, 0x02 | 0x40):
                one = dev.DeviceScene(sc).render_tof(s, sensor, phases=phases, params=pp)
                assert dev.lib().wpt_last_render_passes() == 1
            assert bits_equal(one, two), (variant, phases)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0          # little-endian
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


def test_tof_camera_example_equals_the_python_path(dev, tmp_path):
    exe = str(tmp_path / "tof_camera")
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "tof_camera.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe],
                   check=True, timeout=600)
    w, h, s, mpc = 44, 36, 3, 3
    r = subprocess.run([exe, str(w), str(h), str(s), str(tmp_path), str(mpc)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"time of flight" in r.stdout and b"ground truth" in r.stdout
    sensor = host.tof_sensor()
    ds = dev.DeviceScene(host.tof_scene(w, h, 0))
    planes = ds.render_tof(s, sensor, params=params(mpc, rr=0.0))
    for j in range(4):
        assert bits_equal(read_pfm(str(tmp_path / ("energies-%d.pfm" % j))), planes[j]), j
    # result() of the C++ sensor on its digital numbers against tof_result on the energies: the same distances up to rounding
    result = read_pfm(str(tmp_path / "result.pfm"))
    dist, _, _, _ = dev.tof_result(planes[:, :, :, 0] - planes[:, :, :, 1], 10e6)
    electrons = 0.8 * 880.0 * planes[:, :, :, :2].max(axis=(0, 3)) / 1.98644582 / 10000.0
    lit = (planes[0, :, :, 2] > 0) & (electrons < 0.9 * 100000)        # where no tap saturates
    assert lit.sum() > w * h // 2 and np.allclose(result[:, :, 0][lit], dist[lit], atol=2e-3)
    gt = dev.ground_truth(ds, bits=1 << 11)["camera_space_distances"][:, :, 0]
    words = r.stdout.decode().split("centre pixel: measured distance ")[1].split()
    assert abs(float(words[0]) - result[h // 2, w // 2, 0]) < 1e-4 and abs(float(words[-2]) - gt[h // 2, w // 2]) < 1e-4


def test_phase_from_geometry(dev):
    """The wall and a light of half-diagonal r centred at the camera C, direct light only, no jitter, 10 MHz, four phases in one
    launch, 16 spp.  Every contribution is a path C - P - L with L on the light, so its length lies between 2 |P - C| - r and
    2 |P - C| + r and its phase between the phases of those two; the decoded phasor is a positive mix of them (all within less
    than a quarter turn), so the decoded distance -- half the path -- lies within r / 2 of n_cam |P - C|, plus s = 2^-16 rad of
    phase as a distance for the float32 rounding of the phasor.  n_cam = 1: the camera is in vacuum."""
    w, h, s = 88, 72, 4
    f = 10e6
    sc = host.tof_scene(w, h, 4)
    light = [m for m in materials(sc) if m.type == _abi.MAT_LIGHT_SPOT][0]
    ds = dev.DeviceScene(sc)
    p = params(2, jitter=False)
    sensor = host.tof_sensor(modulation_frequency=f)
    gt = dev.ground_truth(ds, bits=(1 << 11) | (1 << 5), params=p)
    d_true = gt["camera_space_distances"][:, :, 0].astype(np.float64)
    P = gt["camera_space_positions"].astype(np.float64)
    r = float(np.hypot(0.10, 0.05))
    slack = 2.0 ** -16 * C_LIGHT / (4 * np.pi * f)
    # excluded: pixels whose centre ray misses the wall, or whose wall point may lie outside the light's cone for some point
    # of the light (the angle at the light's centre, widened by the angle the light's half-diagonal subtends)
    hit = d_true > 0
    cos_at_centre = np.where(hit, -P[:, :, 2] / np.maximum(d_true, 1e-30), -1.0)
    widened = np.cos(np.minimum(np.arccos(np.clip(cos_at_centre, -1, 1)) + np.arcsin(np.minimum(r / np.maximum(d_true, r), 1.0)), np.pi))
    ok = hit & (widened >= float(light.f[0]))
    assert (~ok).sum() <= 0.05 * w * h, (~ok).sum()
    for kv in kernel_variants(sc):
        with kernel_choice(dev, kv):
            planes = ds.render_tof(s, sensor, params=p)
        dist, amp, _, _ = dev.tof_result(planes[:, :, :, 0] - planes[:, :, :, 1], f)
        assert (amp[ok] > 0).all()
        dev_ = np.abs(dist.astype(np.float64) - 1.0 * d_true)
        print("kernel word %#x: max |measured - true| = %.5f m of %.5f allowed (r / 2 = %.5f)" % (kv, dev_[ok].max(), r / 2 + slack, r / 2))
        assert (dev_[ok] <= r / 2 + slack).all()
        assert d_true[ok].min() > 1.9 and d_true[ok].max() < 15.0 / 2     # far inside the unambiguous range c / (2 f)


def test_fourth_channel_of_the_optical_path_length(dev):
    """A slab of thickness 0.5 with index (1.5, 1.5, 1.5, 1.3) between the camera and a ToF light that faces it, 100 MHz, four
    path components, no jitter, an odd frame: the centre pixel looks along the axis, and only the straight transmitted path
    reaches the light, with opl.w = d1 + 1.3 * 0.5 + d2.  With the first channel's 1.5 the phase would be off by 0.21 rad."""
    w = h = 33
    f = 100e6
    sc = host.tof_scene(w, h, 3)
    sensor = host.tof_sensor(modulation_frequency=f)
    p = params(4, jitter=False)
    d1, d2, thick = 1.0, 1.5, 0.5
    k = 2 * np.pi * f / C_LIGHT
    phi = k * (d1 + float(F32(1.3)) * thick + d2)
    phi_wrong = k * (d1 + 1.5 * thick + d2)
    # the float32 rounding of opl: three additions opl += a * ri, to sums near 1, 1.65 and 3.15, each rounded by at most half a
    # unit in the last place of its sum (2^-24, 2^-24, 2^-23), and the one inexact product 1.3f * a below 1 (2^-25)
    opl_rounding = 2.0 ** -24 + 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -25
    tol = 2.0 ** -16 + k * opl_rounding
    for kv in kernel_variants(sc):
        with kernel_choice(dev, kv):
            planes = dev.DeviceScene(sc).render_tof(4, sensor, params=p)
        a, b = planes[:, h // 2, w // 2, 0].astype(np.float64), planes[:, h // 2, w // 2, 1].astype(np.float64)
        assert (a + b > 0).all()
        ratio = (a - b) / (a + b)
        tau = np.array([float(sensor.tau[j]) for j in range(4)])
        want = 0.75 * np.cos(tau + phi)
        print("kernel word %#x: ratio %s, expected %s, with 1.5: %s" % (kv, ratio, want, 0.75 * np.cos(tau + phi_wrong)))
        print("    max |ratio - expected| = %.3e of %.3e allowed" % (np.abs(ratio - want).max(), 0.75 * tol))
        assert (np.abs(ratio - want) <= 0.75 * tol).all()
        measured = np.arctan2(ratio[3] - ratio[1], ratio[0] - ratio[2]) % (2 * np.pi)
        print("    decoded phase %.7f, expected %.7f: off by %.3e of %.3e allowed" % (measured, phi % (2 * np.pi), abs(measured - phi % (2 * np.pi)), tol))
        assert abs(measured - phi % (2 * np.pi)) <= tol
        miss = abs(measured - phi_wrong % (2 * np.pi))
        assert 0.20 < miss < 0.22, miss
        assert np.abs(ratio - 0.75 * np.cos(tau + phi_wrong)).max() > 0.1


def test_textured_tof_light(dev):
    """LightTof with a texture: the fourth channel times the texture's red value and nothing else.  The twin's LightSpot
    multiplies its x channel by the same red value, so the twin identities hold with the texture in place: exactly at one
    sample (two path components, no jitter: the light's own emission where the camera sees it, the light ray of the first hit
    on the cube, or nothing), within (n + 4) * 2^-24 at 64 spp.  The texture's green lies 40 / 255 above its red in every texel
    (and so between texels), blue as much above green, so a rule that took their average would miss."""
    w, h = 48, 40
    sc, twin, _ = scene_pair(5, w, h, 1)
    light = [m for m in materials(sc) if m.type == _abi.MAT_LIGHT_SPOT][0]
    assert light.flags & 16 and light.tex[0] >= 0 and x_equals_w(sc)
    sensor = host.tof_sensor()
    p = params(2, jitter=False)
    frames = []
    for kv in (0, 0x02):
        with kernel_choice(dev, kv):
            planes = dev.DeviceScene(sc).render_tof(1, sensor, params=p)
            rgb, _ = dev.DeviceScene(twin).render(1, params=p)
        x = rgb[:, :, 0]
        # the light fills 3 x 2 of the 5.04 x 4.2 the frame spans at its distance; its texels show as distinct values
        assert (x > 0).sum() > w * h // 4 and len(np.unique(x)) > 12
        assert (np.abs(rgb[:, :, 1] - x)[x > 0] > 0.01 * x[x > 0]).all()        # green is not red anywhere
        want = np.zeros((h, w), np.float32)
        for iy in range(h):
            for ix in range(w):
                want[iy, ix] = dev.tof_accumulate_host(sensor, 0, float(x[iy, ix]), 0.0, 0, np.zeros(3, np.float32))[2]
        for j in range(4):
            assert bits_equal(planes[j, :, :, 2], want), (kv, j)
        frames.append(planes)
    assert bits_equal(frames[0], frames[1])
    s, mpc = 8, 6
    n = s * s * 2 * mpc
    planes = dev.DeviceScene(sc).render_tof(s, host.tof_sensor(contrast=0.0), phases=[0], params=params(mpc))
    rgb, _ = dev.DeviceScene(twin).render(s, params=params(mpc))
    total = planes[0, :, :, 2].astype(np.float64)
    want = 1000.0 * 144.0 * 0.5 * 1000.0 * rgb[:, :, 0].astype(np.float64)
    err = np.abs(total - want)
    print("64 spp: max relative deviation %.3g of %.3g allowed" % ((err[want > 0] / want[want > 0]).max(), (n + 4) * U))
    assert (want > 0).sum() > w * h // 4 and (err <= (n + 4) * U * want).all()


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_rgb_render_of_a_tof_scene(dev, variant):
    """a ToF light adds 0 to x, y, z: under SensorRGB the scene renders exactly what its twin with a black spot light renders"""
    w, h, s = 40, 32, 3
    sc, twin, times = scene_pair(variant, w, h, 2)
    p = params(6, times=times)
    a, _ = dev.DeviceScene(sc).render(s, params=p)
    b, _ = dev.DeviceScene(twin).render(s, params=p)
    assert bits_equal(a, b) and np.isfinite(a).all()
    assert not a.any()      # and these scenes have no other light
