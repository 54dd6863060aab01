"""The launch's constants in the large form of the kernel with rotated corners (wurblpt_amd/csrc/wpt_blocks.h, LaunchRecordInLds;
wpt_lds_places.h, LAUNCH_RECORD_AT): a launch that reads the material records by LDS address keeps what the new-sample block
reads of the launch -- the origin of the camera's rays, evaluated once (wpt_camera_origin.h), the frustum, the rotation, the
reciprocals of the frame's size and of samples_sqrt, samples_sqrt and randomize_ray_over_pixel -- as a record of four quadwords
in front of the paths' cold words, where the scene ends in front of that place, and reads it with LDS broadcasts.  The words
are the arguments', so every frame here is the oracle's bit for bit; wpt_kernel_launch_record says whether the launch had the
record.  The scheduler's settings stay arguments of their own, and the kernels with the record obey them like the others.

The scenes: the Cornell box (tall box GGX, short box glass) at 64 x 64 and samples_sqrt 4 in the plain large kernel and in the
small form; 640 x 512 at samples_sqrt 2 in the sliced twin, which is launched for pooled frames only; the same box under cameras
whose pose makes the origin more than a copy of the translation; rooms of 16 triangles whose material records leave the record
its four quadwords (151 records) or not (152: they end with the last quadword in front of the cold words)."""
import ctypes as C

import numpy as np
import pytest

from tests import lds_edge_cases as cases
from tests.test_gpu_ordered_boxes import LARGE, ROTATED, SMALL, bits_differing, ran
from tests.test_hit_data_layout import HOTSPOTS, RECORDS, ROOM
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

POOLED = (640, 512)       # 327 680 pixels against 262 144 lanes in flight on an MI355X
BAND = (250, 8)           # eight rows across the boxes
RECORD_QUADS = 4          # wpt_lds_places.h, LAUNCH_RECORD_QUADS


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def render(dev, sc, s, params=None, walk=0, slices=0, variant=0):
    """(frame, what ran, launch record in LDS?) of one launch"""
    ds = dev.DeviceScene(sc)
    try:
        dev.lib().wpt_set_walk(walk)
        dev.lib().wpt_set_launch_config(0, variant)
        dev.set_slices(slices)
        got, _ = ds.render(s, params=params)
        return got, ran(dev), dev.kernel_launch_record()
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_launch_config(0, 0)
        dev.lib().wpt_set_walk(0)
        ds.close()


def reference(oracle, sc, s, params=None, block=None):
    ref, _ = oracle.render(sc, s, params=params, block=block)
    rendered = ref if block is None else ref.reshape(-1, 3)[block[0]:block[0] + block[1]]
    assert np.isfinite(rendered).all() and rendered.mean() > 0.001, float(rendered.mean())
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def cornell(oracle):
    """the Cornell box at 64 x 64 and the oracle's frame at samples_sqrt 4, made once"""
    sc = host.cornell(64, 64, 1, 2)
    return sc, reference(oracle, sc, 4)


def test_the_cornell_box_in_the_plain_large_kernel(dev, cornell):
    sc, ref = cornell
    got, what, record = render(dev, sc, 4)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert record and dev.kernel_materials_in_lds()
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_the_small_form_has_no_record(dev, cornell):
    sc, ref = cornell
    got, what, record = render(dev, sc, 4, walk=dev.WALK_SMALL_WORKGROUPS)
    assert what == ("wpt_pathtrace", ROTATED, SMALL), what
    assert not record
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_hit_data_in_hbm_switches_it_off(dev, cornell):
    """no material records by LDS address, no record: the large form's kernel without parts, which reads the arguments"""
    sc, ref = cornell
    got, what, record = render(dev, sc, 4, walk=dev.WALK_HIT_DATA_IN_HBM)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert not record
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_the_sliced_twin(dev, oracle):
    """a pooled frame: a band of eight rows across the boxes against the oracle, the whole frame against the launch with one lane
    per pixel (the plain kernel)"""
    sc = host.cornell(*POOLED, 1, 2)
    w = POOLED[0]
    ref = reference(oracle, sc, 2, block=(BAND[0] * w, BAND[1] * w))
    band = slice(BAND[0], BAND[0] + BAND[1])
    got, what, record = render(dev, sc, 2, slices=2)
    assert what == ("wpt_pathtrace", ROTATED + ", sliced x2", LARGE) and record, (what, record)
    one_lane_per_pixel, what, record = render(dev, sc, 2, variant=0x10)
    assert what == ("wpt_pathtrace", ROTATED, LARGE) and record, (what, record)
    assert bits_differing(got[band], ref[band]) == 0, bits_differing(got[band], ref[band])
    assert bits_differing(got, one_lane_per_pixel) == 0, bits_differing(got, one_lane_per_pixel)


def posed(name):
    """the Cornell box at 64 x 64 with its camera's pose changed"""
    sc = host.cornell(64, 64, 1, 2)
    cam = sc.camera.contents
    if name in ("negative zero translation", "all three"):
        # the box is symmetric about x = 0 and the camera stands there: the component keeps its value and changes its sign bit
        assert cam.translation[0] == 0.0
        cam.translation[0] = -0.0
        assert np.signbit(np.float32(cam.translation[0]))
    if name in ("rotation", "all three"):
        # turned by 0.1 rad about the world y axis: (0, s, 0, c) * q
        qx, qy, qz, qw = [np.float32(v) for v in cam.rotation]
        s, c = np.float32(np.sin(0.05)), np.float32(np.cos(0.05))
        cam.rotation[0], cam.rotation[1] = float(c * qx + s * qz), float(c * qy + s * qw)
        cam.rotation[2], cam.rotation[3] = float(c * qz - s * qx), float(c * qw - s * qy)
        assert abs(cam.rotation[1]) > 0.01
    if name in ("scaling", "all three"):
        cam.scaling[0], cam.scaling[1], cam.scaling[2] = 2.0, -0.5, 3.0   # 0 * -0.5 is -0
    return sc


@pytest.mark.parametrize("name", ["negative zero translation", "rotation", "scaling", "all three"])
def test_cameras_whose_origin_is_computed(dev, oracle, name):
    sc = posed(name)
    ref = reference(oracle, sc, 4)
    got, what, record = render(dev, sc, 4)
    assert what == ("wpt_pathtrace", ROTATED, LARGE) and record, (what, record)
    assert bits_differing(got, ref) == 0, (name, bits_differing(got, ref))


def test_the_rotation_changes_the_frame(oracle, cornell):
    """(the posed cameras are not the plain one in disguise)"""
    assert bits_differing(oracle.render(posed("rotation"), 4)[0], cornell[1]) > 0


def test_rays_through_the_pixels_centres(dev, oracle):
    """randomize_ray_over_pixel = 0: the block draws nothing for the ray, and the flag is a word of the record"""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    sc = host.cornell(64, 64, 1, 2)
    ref = reference(oracle, sc, 4, params=p)
    got, what, record = render(dev, sc, 4, params=p)
    assert what == ("wpt_pathtrace", ROTATED, LARGE) and record, (what, record)
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)
    assert bits_differing(ref, oracle.render(sc, 4)[0]) > 0


def test_a_batch_of_two_views(dev, oracle):
    """the views' kernel reads each lane's own camera where a wave spans two views: an unchanged path"""
    sc = host.cornell(64, 64, 1, 2)
    cams = [_abi.Camera.from_buffer_copy(sc.camera.contents), _abi.Camera.from_buffer_copy(posed("all three").camera.contents)]
    ds = dev.DeviceScene(sc)
    try:
        frames = ds.render_views(4, cams).cpu().numpy()
    finally:
        ds.close()
    assert not dev.kernel_launch_record()
    for v, cam in enumerate(cams):
        C.memmove(C.addressof(sc.camera.contents), C.addressof(cam), C.sizeof(cam))
        ref = reference(oracle, sc, 4)
        assert bits_differing(frames[v], ref) == 0, (v, bits_differing(frames[v], ref))


def test_a_lens_camera(dev, oracle):
    """a thin lens: the origin is drawn per sample on the lens, in the all-features kernel: an unchanged path"""
    sc = host.cornell(64, 64, 1, 2)
    cam = sc.camera.contents
    cam.lens_radius, cam.focus_dist = 0.05, 3.0
    ref = reference(oracle, sc, 4)
    got, what, record = render(dev, sc, 4)
    assert what[2] == SMALL and not record, (what, record)
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


# wpt_set_launch_config words: byte 0 bits 2-3 pick waitBelow (6, 0, 3, 12), bit 0x20 the separate rounds; byte 1 leaveEighths + 1,
# byte 2 heavyMin + 1, byte 3 leafBias.  The settings' largest values are among them
WORDS = [
    0x08 | (4 << 8) | (25 << 16) | (8 << 24),             # waitBelow 3, leaveEighths 3, heavyMin 24, leafBias 8
    0x2c | (9 << 8) | (2 << 16) | (255 << 24),            # separate rounds, waitBelow 12, leaveEighths 8, heavyMin 1, leafBias 255
    0x04 | (255 << 16),                                   # no kind ever stands back, heavyMin 254: long rounds only when nothing walks
]


@pytest.mark.parametrize("word", WORDS, ids=["0x%08x" % w for w in WORDS])
def test_scheduler_settings_of_the_launch(dev, cornell, word):
    """how a wave schedules its lanes never changes what a lane computes: the oracle's frame under every word"""
    sc, ref = cornell
    got, what, record = render(dev, sc, 4, variant=word)
    assert what == ("wpt_pathtrace", ROTATED, LARGE) and record, (what, record)
    assert bits_differing(got, ref) == 0, (hex(word), bits_differing(got, ref))


# rooms of 16 triangles (31 nodes): hit records and hot spots end at quadword 800 (tests/test_gpu_material_lds.py), the material
# records of 8 quadwords follow, and the record's place is the room's last four quadwords
@pytest.mark.parametrize("materials,fits", [(151, True), (152, False)], ids=["151 records", "152 records"])
def test_rooms_on_either_side_of_the_records_place(dev, oracle, materials, fits):
    sc = host.lds_edge_scene(16, materials, 0, cases.SEED[16], cases.W, cases.H)
    d = sc.d
    assert (d.node_count, d.tri_count, d.material_count, d.hotspot_count) == (31, 16, materials, 2)
    by_lds, at, quads = dev.material_places(d.node_count, d.tri_count, d.material_count, False, 0, d.hotspot_count)
    assert by_lds and at == 800 and quads == 800 + 8 * materials
    assert (quads <= ROOM - RECORD_QUADS) == fits and quads <= ROOM
    ref = reference(oracle, sc, cases.S)
    got, what, record = render(dev, sc, cases.S)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert dev.kernel_hit_data() == RECORDS | HOTSPOTS and dev.kernel_materials_in_lds()
    assert record == fits
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)
