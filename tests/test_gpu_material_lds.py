"""The material records by LDS address (wurblpt_amd/csrc/wpt_lds_places.h, materialPlaces): a launch in the large form of the
kernel with rotated corners whose kernel reads hit records and hot spots from LDS keeps the material records there too -- behind
the corners where the kernel choice has them in LDS anyway, else behind the hit data where they end in front of the paths' cold
words -- and its long round fetches a hit's material, and a light ray's light, with LDS instructions at an offset from the scene's
start.  The records are the scene's own, word for word, and the arithmetic is every other kernel's, so every frame here is the
oracle's bit for bit; wpt_kernel_materials_in_lds says what the launch had, and WPT_WALK_HIT_DATA_IN_HBM switches it off with
the parts of a hit's data.

The scenes: the Cornell box with the tall box GGX and the short box glass beside the Lambertian walls, the light seen directly
and reached by light rays, 64 x 64 pixels at samples_sqrt 4 in the plain large kernel; 640 x 512 in its sliced twin, which is
launched for pooled frames only; and rooms of 16 triangles whose number of records puts them on either side of the room's end
(152 records end with the last quadword in front of the cold words, 153 do not fit) and behind the corners (34).  The counts are
checked with the placement function itself (wpt_material_places), never taken for granted."""
import numpy as np
import pytest

from tests import lds_edge_cases as cases
from tests.test_gpu_ordered_boxes import LARGE, ROTATED, bits_differing, ran
from tests.test_hit_data_layout import HOTSPOTS, RECORDS, ROOM
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

POOLED = (640, 512)       # 327 680 pixels against 262 144 lanes in flight on an MI355X
BAND = (250, 8)           # eight rows across the boxes


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def verdict(dev, sc):
    """(by LDS address?, first quadword, quadwords of the scene) from the placement function for the scene's own counts and its
    kernel choice; no triangle of these scenes is transformed"""
    d = sc.d
    chosen = cases.choice(sc, 0)
    assert chosen[1] == ROTATED, chosen
    assert not any(d.tri_geom[i].flags & 4 for i in range(d.tri_count))
    return dev.material_places(d.node_count, d.tri_count, d.material_count, bool(chosen[4] & cases.LDS_MATERIALS), 0, d.hotspot_count)


def render(dev, sc, s, walk=0, slices=0, variant=0):
    """(frame, what ran, parts of a hit's data in LDS, materials by LDS address) of one launch"""
    ds = dev.DeviceScene(sc)
    try:
        dev.lib().wpt_set_walk(walk)
        dev.lib().wpt_set_launch_config(0, variant)
        dev.set_slices(slices)
        got, _ = ds.render(s)
        return got, ran(dev), dev.kernel_hit_data(), dev.kernel_materials_in_lds()
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_launch_config(0, 0)
        dev.lib().wpt_set_walk(0)
        ds.close()


@pytest.fixture(scope="module")
def cornell(oracle):
    """the Cornell box at 64 x 64 and the oracle's frame at samples_sqrt 4, made once.  The frame shows what the test is about: the
    light itself (pixels brighter than any surface), and the three kinds of material among the records the hits name"""
    sc = host.cornell(64, 64, 1, 2)
    ref, _ = oracle.render(sc, 4)
    assert np.isfinite(ref).all() and ref.mean() > 0.001
    d = sc.d
    types = {int(d.materials[int(d.tri_geom[t].material)].type) for t in range(int(d.tri_count))}
    assert {_abi.MAT_LAMBERTIAN, _abi.MAT_GGX, _abi.MAT_GLASS, _abi.MAT_LIGHT_DIFFUSE} <= types, types
    assert d.hotspot_count == 2                    # light rays are sent, and end in blockNeeEnd at the light's record
    assert (ref.max(axis=2) >= 4.0).sum() >= 8     # the light is hit directly: pixels that show what it emits
    ref.setflags(write=False)
    return sc, ref


def test_the_cornell_box_in_the_plain_large_kernel(dev, cornell):
    sc, ref = cornell
    fits, at, quads = verdict(dev, sc)
    assert (fits, at, quads) == (True, 1772, 1820)       # six records behind the hot spots
    got, what, parts, by_lds = render(dev, sc, 4)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert parts == RECORDS | HOTSPOTS and by_lds
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_hit_data_in_hbm_switches_it_off(dev, cornell):
    sc, ref = cornell
    got, what, parts, by_lds = render(dev, sc, 4, walk=dev.WALK_HIT_DATA_IN_HBM)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert parts == 0 and not by_lds
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_small_workgroups_report_nothing(dev, cornell):
    """the kernels of 256 lanes read the records through the scene's array, and say so"""
    sc, ref = cornell
    got, what, parts, by_lds = render(dev, sc, 4, walk=dev.WALK_SMALL_WORKGROUPS)
    assert what[2] != LARGE and parts == 0 and not by_lds, (what, parts, by_lds)
    assert bits_differing(got, ref) == 0, bits_differing(got, ref)


def test_the_sliced_twin(dev, oracle):
    """a pooled frame: a band of eight rows across the boxes against the oracle, the whole frame against the launch with one lane
    per pixel (the plain kernel)"""
    sc = host.cornell(*POOLED, 1, 2)
    w = POOLED[0]
    ref, _ = oracle.render(sc, 2, block=(BAND[0] * w, BAND[1] * w))
    band = slice(BAND[0], BAND[0] + BAND[1])
    assert np.isfinite(ref).all() and ref[band].mean() > 0.001
    got, what, parts, by_lds = render(dev, sc, 2, slices=2)
    assert what == ("wpt_pathtrace", ROTATED + ", sliced x2", LARGE), what
    assert parts == RECORDS | HOTSPOTS and by_lds
    one_lane_per_pixel, what, parts, by_lds = render(dev, sc, 2, variant=0x10)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert parts == RECORDS | HOTSPOTS and by_lds
    assert bits_differing(got[band], ref[band]) == 0, bits_differing(got[band], ref[band])
    assert bits_differing(got, one_lane_per_pixel) == 0, bits_differing(got, one_lane_per_pixel)


# rooms of 16 triangles (31 nodes): the node copies end at quadword 672, 16 hit records at 784, two hot spots at 800, and 1216
# quadwords are left: 152 records.  (records, by LDS address?, where, behind the corners?)
ROOMS = [
    (34, True, 64 + 144, True),         # in LDS behind the corners anyway (tests/lds_edge_cases.py, PLAIN): read there
    (35, True, None, False),            # the first count that the kernel choice leaves in HBM: behind the hot spots
    (152, True, None, False),           # the last count that fits: the records end with the room's last quadword
    (153, False, None, False),          # the first that does not: the launch falls back to the kernel that reads the scene's array
]


@pytest.mark.parametrize("materials,fits,where,behind", ROOMS, ids=["%d records" % r[0] for r in ROOMS])
def test_rooms_on_either_side_of_the_end(dev, oracle, materials, fits, where, behind):
    sc = host.lds_edge_scene(16, materials, 0, cases.SEED[16], cases.W, cases.H)
    d = sc.d
    assert (d.node_count, d.tri_count, d.material_count, d.hotspot_count) == (31, 16, materials, 2)
    assert bool(cases.choice(sc, 0)[4] & cases.LDS_MATERIALS) == behind
    got_fits, at, quads = verdict(dev, sc)
    assert got_fits == fits, (got_fits, at, quads)
    if behind:
        assert at == where and quads <= ROOM
    elif fits:
        assert at == 800 and quads == 800 + 8 * materials <= ROOM
        assert (quads == ROOM) == (materials == 152)
    else:
        assert at == 800 and quads == 800 and 800 + 8 * materials > ROOM >= 800 + 8 * (materials - 1)
    ref, _ = oracle.render(sc, cases.S)
    assert np.isfinite(ref).all() and ref.mean() > 0.001
    frame, what, parts, by_lds = render(dev, sc, cases.S)
    assert what == ("wpt_pathtrace", ROTATED, LARGE), what
    assert parts == RECORDS | HOTSPOTS and by_lds == fits, (parts, by_lds)
    assert bits_differing(frame, ref) == 0, bits_differing(frame, ref)
