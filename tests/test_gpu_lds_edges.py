"""The kernels that keep the scene in LDS at the edges of their layout (tests/lds_edge_cases.py, host.lds_edge_scene): scenes whose
nodes, corners and material records take the loops that copy them into LDS round once more or exactly fill what a launch may
ask for, and their neighbours one record or one triangle further, where the records stay in HBM, the rotated copies no longer
fit or the scene itself leaves LDS.  An offset or a bound that is off by one there reads zeros or a neighbour's record and
faults nothing: every frame is compared bit for bit with the oracle's (the time-of-flight planes, which the oracle does not
have, with the kernel that fetches the scene from HBM and through a twin scene with the oracle), and every launch must report
the kernel and form that wpt_kernel_choice names for the scene's own counts, which must be the side of the edge the case is
about."""
import numpy as np
import pytest

from wurblpt_amd import _abi, host

from tests import lds_edge_cases as cases
from tests.test_gpu_rotated import axis_cameras
from tests.test_gpu_sliced import H as BIG_H, W as BIG_W
from tests.test_gpu_transient import check_bins

pytestmark = pytest.mark.gpu

S = cases.S


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


@pytest.fixture(scope="module")
def on_device(dev):
    """the DeviceScene of a case, uploaded once"""
    cache = {}

    def get(t, m, light=0, width=cases.W, height=cases.H):
        key = (t, m, light, width, height)
        if key not in cache:
            sc = cases.scene(*key)
            cache[key] = (sc, dev.DeviceScene(sc))
        return cache[key]
    yield get
    for _, ds in cache.values():
        ds.close()


@pytest.fixture(scope="module")
def reference(oracle):
    """the oracle's frame of a case from its own camera, rendered once and read-only"""
    cache = {}

    def get(t, m, light=0, s=S):
        key = (t, m, light, s)
        if key not in cache:
            cache[key] = oracle.render(cases.scene(t, m, light), s)[0]
            cache[key].setflags(write=False)
        return cache[key]
    return get


def bits_differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def ran(dev, chosen, suffix=""):
    """the launch behind us ran the kernel wpt_kernel_choice names, in its form"""
    name, form = dev.lib().wpt_kernel_name().decode(), dev.lib().wpt_kernel_form().decode()
    assert (name, form) == (chosen[0], chosen[1] + suffix), (name, form, chosen)


class walk:
    def __init__(self, dev, flags):
        self.dev, self.flags = dev, flags

    def __enter__(self):
        self.dev.lib().wpt_set_walk(self.flags)

    def __exit__(self, *a):
        self.dev.lib().wpt_set_walk(0)


class launch_config:
    def __init__(self, dev, variant):
        self.dev, self.variant = dev, variant

    def __enter__(self):
        self.dev.lib().wpt_set_launch_config(0, self.variant)

    def __exit__(self, *a):
        self.dev.lib().wpt_set_launch_config(0, 0)


@pytest.mark.parametrize("t,m", sorted(cases.PLAIN))
def test_plain_frames_with_the_materials_behind_the_rotated_copies(dev, on_device, reference, t, m):
    sc, ds = on_device(t, m)
    ref = reference(t, m)
    assert cases.side(sc, cases.choice(sc, dev.SENSOR_FRAME)) == cases.PLAIN[(t, m)]
    for flags in (0, dev.WALK_SELECT_CORNERS, dev.WALK_NO_FOLD):
        chosen = cases.choice(sc, dev.SENSOR_FRAME, walk=flags)
        if flags == dev.WALK_SELECT_CORNERS:
            assert cases.side(sc, chosen).startswith("select, materials in LDS")
        with walk(dev, flags):
            got, _ = ds.render(S)
            ran(dev, chosen)
        assert bits_differing(got, ref) == 0, (flags, bits_differing(got, ref))


@pytest.mark.parametrize("t,m", [(16, 34), (36, 2)])
def test_every_rotations_copy_is_read(dev, oracle, on_device, t, m):
    """from the middle of the room along every axis in both directions: camera rays of every largest component"""
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_FRAME)
    assert cases.side(sc, chosen) == cases.PLAIN[(t, m)] and chosen[1] == "rotated corners"
    saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
    try:
        for label, cam in axis_cameras(sc)[1:]:
            sc.camera[0] = cam
            ref, _ = oracle.render(sc, S)
            got, _ = ds.render(S)
            ran(dev, chosen)
            assert ref.any() and bits_differing(got, ref) == 0, (label, bits_differing(got, ref))
    finally:
        sc.camera[0] = saved


def sensor_frame(dev, oracle, on_device, reference, t, m):
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_FRAME, walk=dev.WALK_SELECT_CORNERS)
    assert cases.side(sc, chosen) == cases.SENSORS[(t, m)]
    with walk(dev, dev.WALK_SELECT_CORNERS):
        got, _ = ds.render(S)
        ran(dev, chosen)
    assert bits_differing(got, reference(t, m)) == 0


def sensor_transient(dev, oracle, on_device, reference, t, m):
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_TRANSIENT)
    assert cases.side(sc, chosen) == cases.SENSORS[(t, m)]
    edges = dev.uniform_edges(0.0, 1.25, 8)                 # the room is 2 wide: paths of up to 10
    frame, bins = ds.render_transient(S, edges)
    ran(dev, chosen)
    assert sum(int(bins[k].any()) for k in range(8)) >= 4
    check_bins(oracle, sc, S, edges, bins)
    assert bits_differing(frame, reference(t, m)) == 0


def sensor_views(dev, oracle, on_device, reference, t, m):
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_VIEWS)
    assert cases.side(sc, chosen) == cases.SENSORS[(t, m)]
    cams = [_abi.Camera.from_buffer_copy(sc.camera.contents), host.camera_looking_at(sc, (0.6, 0.4, 0.9), (-0.3, -0.5, -0.8)),
            host.camera_looking_at(sc, (-0.8, 0.7, -0.1), (0.9, -0.9, -0.4))]
    views = ds.render_views(S, cams).cpu().numpy()
    ran(dev, chosen)
    plain, _ = ds.render(S)
    assert bits_differing(views[0], plain) == 0 and bits_differing(views[0], reference(t, m)) == 0
    saved = cams[0]
    try:
        for v in (1, 2):
            sc.camera[0] = cams[v]
            ref, _ = oracle.render(sc, S)
            assert ref.any() and bits_differing(views[v], ref) == 0, v
    finally:
        sc.camera[0] = saved


def sensor_adaptive(dev, oracle, on_device, reference, t, m):
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_ADAPTIVE)
    assert cases.side(sc, chosen) == cases.SENSORS[(t, m)]
    counts = ((np.arange(cases.W)[None, :] + 3 * np.arange(cases.H)[:, None]) % 4).astype(np.uint16)     # 0 .. 3 rows of strata
    frame, moments = ds.render_adaptive(counts, with_moments=True)
    ran(dev, chosen)
    frame, moments = frame.cpu().numpy(), moments.cpu().numpy()
    with launch_config(dev, 0x01):                          # the same map through the kernel that fetches the scene from HBM
        hbm_frame, hbm_moments = ds.render_adaptive(counts, with_moments=True)
        assert "scene in LDS" not in dev.lib().wpt_kernel_name().decode()
    assert bits_differing(frame, hbm_frame.cpu().numpy()) == 0 and bits_differing(moments, hbm_moments.cpu().numpy()) == 0
    assert not frame[counts == 0].any() and not moments[counts == 0].any()
    for n in (1, 2, 3):
        sel = counts == n
        plain, _ = ds.render(n)
        ref = reference(t, m, 0, n)
        assert bits_differing(frame[sel], plain[sel]) == 0 and bits_differing(frame[sel], ref[sel]) == 0, n
    assert bits_differing(moments[counts == 1], frame[counts == 1] * frame[counts == 1]) == 0
    assert (moments >= 0.0).all() and (moments >= 0.999 * frame * frame).all() and moments.any()


def sensor_tof(dev, oracle, on_device, reference, t, m):
    """light 2 (cases.TOF has the numbers of records).  All phases in one launch are, plane by plane, the planes of the kernel that
    fetches the scene from HBM; and with one sample through the pixel's centre and two path components a pixel has one
    contribution at most, the light ray of its first hit, which is the x channel of the twin scene's frame under the oracle
    (light 1: a LightSpot of the ToF light's radiance in all channels): `total` is the sensor's rule applied to it once."""
    m = max(m, 4)
    sc, ds = on_device(t, m, 2)
    chosen = cases.choice(sc, dev.SENSOR_TOF)
    assert cases.side(sc, chosen) == cases.TOF[(t, m)]
    sensor = host.tof_sensor(phase_image_count=4, modulation_frequency=20e6)
    planes = ds.render_tof(S, sensor)
    ran(dev, chosen)
    with launch_config(dev, 0x02):
        hbm = ds.render_tof(S, sensor)
        assert dev.lib().wpt_kernel_name() == b"wpt_pathtrace, time of flight, all features"
    assert planes[:, :, :, 2].any() and bits_differing(planes, hbm) == 0
    assert (planes[0, :, :, 0] != planes[0, :, :, 1]).any()                                 # the light is modulated
    for j in range(1, 4):
        assert bits_differing(planes[j, :, :, 2], planes[0, :, :, 2]) == 0
    # the twin: every record but the light's front side is the same, and attenuates the fourth channel like the first
    twin = cases.scene(t, m, 1)
    for i in range(m):
        a, b = sc.d.materials[i], twin.d.materials[i]
        if i != m - 3:
            assert bytes(a) == bytes(b)
        if a.type in (_abi.MAT_LAMBERTIAN, _abi.MAT_GGX, _abi.MAT_GLASS):
            assert a.v[0][0] == a.v[0][3] and (a.type != _abi.MAT_LAMBERTIAN or a.flags & 1)
    p = host.default_params()
    p.max_path_components, p.randomize_ray_over_pixel = 2, 0
    x = oracle.render(twin, 1, params=p)[0][:, :, 0]
    # the identity says something where the twin shows light: with one sample and the light ray alone that is where the first
    # hit sees the ceiling light unoccluded, a tenth of the pixels in the most cluttered room; a twentieth is asked for
    assert (x > 0).sum() >= cases.W * cases.H // 20, "the twin is dark"
    one = ds.render_tof(1, sensor, params=p)
    ran(dev, chosen)
    want = np.zeros_like(x)
    for iy in range(x.shape[0]):
        for ix in range(x.shape[1]):
            want[iy, ix] = dev.tof_accumulate_host(sensor, 0, float(x[iy, ix]), 0.0, 0, np.zeros(3, np.float32))[2]
    for j in range(4):
        assert bits_differing(one[j, :, :, 2], want) == 0, j


SENSOR_TESTS = {"frame": sensor_frame, "transient": sensor_transient, "views": sensor_views, "adaptive": sensor_adaptive, "tof": sensor_tof}


@pytest.mark.parametrize("t,m", sorted(cases.SENSORS))
@pytest.mark.parametrize("sensor", sorted(SENSOR_TESTS))
def test_every_kernel_that_does_not_rotate(dev, oracle, on_device, reference, sensor, t, m):
    SENSOR_TESTS[sensor](dev, oracle, on_device, reference, t, m)


@pytest.mark.parametrize("t,m,flags", [(183, 2, 0), (36, 2, 0), (36, 2, 16)])
def test_the_sliced_twins(dev, oracle, on_device, t, m, flags):
    """a frame just above the device's lanes in two units per pixel: the largest scene in LDS (select form: its copies do not fit)
    and the last one whose copies fit, in both forms"""
    import torch
    assert flags in (0, dev.WALK_SELECT_CORNERS)
    sc, ds = on_device(t, m, 0, BIG_W, BIG_H)
    chosen = cases.choice(sc, dev.SENSOR_FRAME, walk=flags)
    want = "select, materials in HBM" if t == 183 else "select, materials in LDS in 1 trip" if flags else cases.PLAIN[(t, m)]
    assert cases.side(sc, chosen) == want
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = dev.launch_plan(dev.SENSOR_FRAME, False, cases.need(sc), True, BIG_W * BIG_H, S, cus, slices=2)
    assert plan["strategy"] == "sliced" and plan["units"] == 2
    rows = (316, 8)
    ref, _ = oracle.render(sc, S, block=(rows[0] * BIG_W, rows[1] * BIG_W))
    band = slice(rows[0], rows[0] + rows[1])
    assert (ref[band] != 0).any(axis=2).mean() >= 0.5
    try:
        dev.lib().wpt_set_walk(flags)
        dev.set_slices(1)
        whole, _ = ds.render(S)
        ran(dev, chosen)
        dev.set_slices(2)
        got, _ = ds.render(S)
        ran(dev, chosen, ", sliced x2")
        taken, continued = dev.last_slice_stats()
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_walk(0)
    assert taken + continued == BIG_W * BIG_H
    assert bits_differing(got[band], ref[band]) == 0
    assert bits_differing(got, whole) == 0


def test_a_progressive_session_of_the_largest_scene(dev, on_device, reference):
    import torch
    t, m = 183, 2
    sc, ds = on_device(t, m)
    chosen = cases.choice(sc, dev.SENSOR_FRAME)
    assert cases.side(sc, chosen) == cases.SENSORS[(t, m)]
    frame = torch.zeros((cases.H, cases.W, 3), dtype=torch.float32, device="cuda")
    session = ds.progressive(S)
    try:
        assert session.rows_total == S
        for stage in range(S):
            assert session.advance(1, frame) == stage + 1
            torch.cuda.synchronize()
            ds.check()
            ran(dev, chosen)
        assert session.finished
    finally:
        session.close()
    once, _ = ds.render(S)
    ran(dev, chosen)
    assert bits_differing(frame.cpu().numpy(), once) == 0 and bits_differing(once, reference(t, m)) == 0
