"""A hit's data in LDS (wurblpt_amd/csrc/wpt_lds_places.h): the large form of the kernel with rotated corners keeps, behind its
node copies, a record per triangle with the shading attributes and the instance, material and flag words, the hot spots with
their faces, and the normal matrices of the instances that transformed triangles name -- each part where it still fits in front
of the paths' cold words.  finishHit, the light sample and the light-pdf loop then read LDS where every other kernel reads
global memory; the values and the arithmetic are the same, so every frame here is the oracle's bit for bit and the frame of the
same launch under WPT_WALK_HIT_DATA_IN_HBM, and wpt_kernel_hit_data says which parts the launch had in LDS.  The parts are
template arguments: the launch runs the kernel for all three, for records and hot spots, or for none, the largest that fits.

The small frames run the plain large unit.  Its sliced twin is launched for pooled frames only, which have more pixels than the
device has lanes in flight (tests/test_gpu_sliced.py): one such frame at the end, a band of it against the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

from wurblpt_amd import _abi, host

from tests import lds_edge_cases as cases
from tests.test_gpu_ordered_boxes import LARGE, ROTATED, bits_differing, ran, wrapped
from tests.test_hit_data_layout import HOTSPOTS, NORMALS, RECORDS, ROOM, places

pytestmark = pytest.mark.gpu

TRI_TRANSFORM = 4


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def both_places(dev, oracle, sc, samples_sqrt, parts, form=ROTATED):
    """renders the scene with the hit's data where the launch puts it and under WPT_WALK_HIT_DATA_IN_HBM, both in the large form;
    the first must have had `parts` in LDS, and both frames are the oracle's"""
    ref, _ = oracle.render(sc, samples_sqrt)
    ds = dev.DeviceScene(sc)
    try:
        got, _ = ds.render(samples_sqrt)
        assert ran(dev) == ("wpt_pathtrace", form, LARGE), ran(dev)
        assert dev.kernel_hit_data() == parts, dev.kernel_hit_data()
        dev.lib().wpt_set_walk(dev.WALK_HIT_DATA_IN_HBM)
        hbm, _ = ds.render(samples_sqrt)
        assert ran(dev) == ("wpt_pathtrace", form, LARGE), ran(dev)
        assert dev.kernel_hit_data() == 0
    finally:
        dev.lib().wpt_set_walk(0)
        ds.close()
    assert ref.any()
    assert bits_differing(got, hbm) == 0 and bits_differing(got, ref) == 0 and bits_differing(hbm, ref) == 0


def counts(sc, instances):
    """the layout function's verdict for the scene's counts (material records in LDS as wpt_kernel_choice says)"""
    d = sc.d
    chosen = cases.choice(sc, 0)
    assert chosen[1] == ROTATED, chosen
    return places(d.node_count, d.tri_count, d.material_count if chosen[4] & cases.LDS_MATERIALS else 0, instances, d.hotspot_count)


def transformed(sc, instances=None):
    """every triangle of the scene becomes one of a transformed instance (WPT_TRI_TRANSFORM: its normals and tangents go through
    the instance's normal matrix; the positions of a description are transformed already), each instance with a matrix of its
    own.  `instances`: the length of the instance array, the last triangle naming the last one"""
    d = sc.d
    n = int(d.instance_count)
    total = n if instances is None else instances
    assert total >= n
    array = (_abi.Instance * total)()
    for i in range(total):
        array[i] = _abi.Instance.from_buffer_copy(d.instances[i % n])
        a, b, s = 0.05 + 0.01 * (i % 7), 0.03 * (i % 5), 1.0 + 0.125 * (i % 3)
        ca, sa, cb, sb = math.cos(a), math.sin(a), math.cos(b), math.sin(b)
        # a rotation about y, then one about x, scaled: column major
        m = [[ca, 0.0, sa], [sa * sb, cb, -ca * sb], [-sa * cb, sb, ca * cb]]
        for col in range(3):
            for row in range(3):
                array[i].N[3 * col + row] = s * m[row][col]
    last = int(d.tri_count) - 1
    if total > n:
        array[total - 1] = array[d.tri_geom[last].instance]
    sc.transformed_instances = array      # (the description points into it)
    d.instances = C.cast(array, type(d.instances))
    d.instance_count = total
    for t in range(int(d.tri_count)):
        d.tri_geom[t].flags |= TRI_TRANSFORM
    if total > n:
        d.tri_geom[last].instance = total - 1
    return sc


def test_the_cornell_box(dev, oracle):
    """the bench scene, tall box GGX and short box glass: records and hot spots in LDS, and no normal matrix, because no triangle
    of it is transformed"""
    both_places(dev, oracle, host.cornell(64, 64, 1, 2), 4, RECORDS | HOTSPOTS)


def test_texture_coordinates_and_tangents_from_the_record(dev, oracle):
    """a mesh whose triangles have texture coordinates and tangents flagged and set: both are interpolated from quadwords 2 .. 5
    of the LDS record"""
    sc = host.cornell(48, 48, 1, 2)
    d = sc.d
    rng = np.random.default_rng(7)
    for t in range(int(d.tri_count)):
        assert d.tri_geom[t].flags & 3 == 3       # WPT_TRI_HAVE_TEXCOORDS | WPT_TRI_HAVE_TANGENTS
        a = d.tri_attr[t]
        for tc in (a.tc0, a.tc1, a.tc2):
            tc[0], tc[1] = rng.random(2)
        n = np.array([a.n0[:], a.n1[:], a.n2[:]], np.float64)
        for k, tan in enumerate((a.t0, a.t1, a.t2)):
            v = np.cross(n[k], rng.standard_normal(3))
            tan[0], tan[1], tan[2] = v / np.linalg.norm(v)
    both_places(dev, oracle, sc, 3, RECORDS | HOTSPOTS)


def test_transformed_instances(dev, oracle):
    """every triangle is transformed: the normal matrices of all 18 instances follow the hot spots in LDS"""
    sc = transformed(host.cornell(48, 48, 1, 2))
    assert counts(sc, 18)["parts"] == RECORDS | HOTSPOTS | NORMALS
    both_places(dev, oracle, sc, 3, RECORDS | HOTSPOTS | NORMALS)


def test_five_hot_spots_one_of_them_transformed(dev, oracle):
    """the light's two triangles as five hot spots, the third with `transform` set and a matrix that moves and stretches it: the
    light sample reads M's four columns from LDS, the pdf loop goes round five times"""
    sc = host.cornell(48, 48, 1, 2)
    d = sc.d
    assert d.hotspot_count == 2
    spots = (_abi.Hotspot * 5)()
    for k in range(5):
        spots[k] = _abi.Hotspot.from_buffer_copy(d.hotspots[k % 2])
    spots[2].transform = 1
    m = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.875, 0.0, 0.015625, -0.0078125, 0.03125, 1.0]    # column major
    for k in range(16):
        spots[2].M[k] = m[k]
    sc.five_hot_spots = spots
    d.hotspots = C.cast(spots, type(d.hotspots))
    d.hotspot_count = 5
    both_places(dev, oracle, sc, 3, RECORDS | HOTSPOTS)


def test_normal_matrices_that_do_not_fit(dev, oracle):
    """sized by the layout function: the smallest instance array whose matrices end behind the cold words.  Records and hot
    spots are in LDS, the matrices stay in HBM"""
    sc = host.cornell(32, 32, 1, 2)
    fits = counts(sc, 18)
    assert fits["parts"] == 7
    n = (ROOM - fits["normals_at"]) // 3 + 1
    sc = transformed(sc, n)
    assert counts(sc, n - 1)["parts"] == 7 and counts(sc, n - 1)["quads"] <= ROOM
    assert counts(sc, n)["parts"] == RECORDS | HOTSPOTS
    both_places(dev, oracle, sc, 2, RECORDS | HOTSPOTS)


def test_a_scene_whose_node_copies_leave_no_room(dev, oracle):
    """16 triangles under so many nodes that the eight node arrays end within 112 quadwords of the cold words: the launch takes
    the large form and keeps all of a hit's data in HBM (the hot spots alone would fit: the records come first)"""
    wraps = next(w for w in range(60) if counts_of(31 + 2 * w)["node_copies_end"] + 7 * 16 > ROOM)
    sc = wrapped(host.lds_edge_scene(16, 2, 0, cases.SEED[16], cases.W, cases.H), wraps)
    verdict = counts(sc, 0)
    assert sc.d.tri_count == 16 and verdict["parts"] == 0 and verdict["node_copies_end"] <= ROOM, verdict
    assert verdict["node_copies_end"] + 8 * sc.d.hotspot_count <= ROOM
    both_places(dev, oracle, sc, cases.S, 0)


def counts_of(nodes):
    return places(nodes, 16, 0, 0, 2)


def test_the_sliced_twin(dev, oracle):
    """more pixels than the device has lanes in flight: the pool hands them out in two units to the large form's sliced twin, with
    records, hot spots and normal matrices in LDS; a band of the frame against the oracle, the whole frame against the same
    launch under WPT_WALK_HIT_DATA_IN_HBM"""
    from tests.test_gpu_sliced import H, W
    sc = transformed(host.cornell(W, H, 1, 2))
    rows = (H // 2 - 4, 8)
    ref, _ = oracle.render(sc, 2, block=(rows[0] * W, rows[1] * W))
    band = slice(rows[0], rows[0] + rows[1])
    ds = dev.DeviceScene(sc)
    try:
        dev.set_slices(2)
        got, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED + ", sliced x2", LARGE), ran(dev)
        assert dev.kernel_hit_data() == RECORDS | HOTSPOTS | NORMALS
        dev.lib().wpt_set_walk(dev.WALK_HIT_DATA_IN_HBM)
        hbm, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED + ", sliced x2", LARGE), ran(dev)
        assert dev.kernel_hit_data() == 0
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_walk(0)
        ds.close()
    assert ref[band].any() and bits_differing(got[band], ref[band]) == 0
    assert bits_differing(got, hbm) == 0
