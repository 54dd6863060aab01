"""The large form of the kernel with rotated corners: one workgroup of 1024 lanes per compute unit, the node array in LDS once
per sign octant of a ray's direction, and a box test that sorts nothing (wurblpt_amd/csrc/wpt_pathtrace_body.inc.h, ldsStep;
wpt_scene_layout.h, orderedBoxCopies).  Every frame here is the oracle's bit for bit and the frame of the same launch under
WPT_WALK_SMALL_WORKGROUPS; wpt_kernel_workgroup says which form ran.  Scenes whose launch cannot take the large form -- the
request does not fit a compute unit's LDS, a box of the tree has lo > hi -- render with workgroups of 256 lanes as before."""
import ctypes as C

import numpy as np
import pytest

from wurblpt_amd import _abi, host

from tests import lds_edge_cases as cases
from tests.test_ordered_boxes import large_request

pytestmark = pytest.mark.gpu

ROTATED = "rotated corners"
LARGE, SMALL = (1024, True), (256, False)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def ran(dev):
    return dev.lib().wpt_kernel_name().decode(), dev.lib().wpt_kernel_form().decode(), dev.kernel_workgroup()


def both_forms(dev, sc, samples_sqrt, params=None, expect=LARGE, form=ROTATED):
    """(frame of the default launch, frame under WPT_WALK_SMALL_WORKGROUPS); the first ran in the form `expect`, the second at 256 lanes"""
    ds = dev.DeviceScene(sc)
    try:
        got, _ = ds.render(samples_sqrt, params=params)
        assert ran(dev) == ("wpt_pathtrace", form, expect), ran(dev)
        dev.lib().wpt_set_walk(dev.WALK_SMALL_WORKGROUPS)
        small, _ = ds.render(samples_sqrt, params=params)
        assert ran(dev) == ("wpt_pathtrace", form, SMALL), ran(dev)
    finally:
        dev.lib().wpt_set_walk(0)
        ds.close()
    return got, small


def test_cornell_in_the_large_form(dev, oracle):
    sc = host.cornell(64, 64, 1, 2)
    ref, _ = oracle.render(sc, 4)
    got, small = both_forms(dev, sc, 4)
    assert ref.any() and bits_differing(got, ref) == 0 and bits_differing(small, ref) == 0


@pytest.mark.parametrize("t,m", [(16, 34), (32, 8), (36, 2)])
def test_scenes_on_the_capacity_edges(dev, oracle, t, m):
    """with the material records in LDS in two trips and in one, and in HBM behind the largest tree whose rotated copies fit"""
    sc = cases.scene(t, m)
    ref, _ = oracle.render(sc, cases.S)
    got, small = both_forms(dev, sc, cases.S)
    assert ref.any() and bits_differing(got, ref) == 0 and bits_differing(small, ref) == 0


def test_a_camera_that_looks_down_an_axis(dev, oracle):
    """Rays through the pixels' centres of an odd-sized frame: the centre column and row have a direction component of exactly
    zero and carry RAY_MAY_NAN.  Such a ray stays unmirrored on copy 0, and every lane of its group takes the sorting test with
    the check for NaN, the mirrored ones on their own copies."""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    sc = host.cornell(33, 33, 1, 2)
    root = sc.d.nodes[0]
    mid = 0.5 * (np.array(root.lo[:], np.float64) + np.array(root.hi[:], np.float64))
    for axis, sign in ((0, 1.0), (2, -1.0)):
        d = np.zeros(3)
        d[axis] = sign
        sc.camera[0] = host.camera_looking_at(sc, mid, mid + d)
        ref, _ = oracle.render(sc, 2, p)
        got, small = both_forms(dev, sc, 2, params=p)
        assert ref.any() and bits_differing(got, ref) == 0 and bits_differing(small, ref) == 0, axis


def wrapped(sc, wraps):
    """the scene's tree under `wraps` more roots, each an inner node with the old root's box whose first child is an empty node:
    more nodes, the same triangles"""
    d = sc.d
    n = int(d.node_count)
    old = [_abi.BvhNode.from_buffer_copy(d.nodes[i]) for i in range(n)]
    nodes = (_abi.BvhNode * (n + 2 * wraps))()
    for k in range(wraps):
        inner, empty = nodes[2 * k], nodes[2 * k + 1]
        inner.lo, inner.hi, inner.kind, inner.link = old[0].lo, old[0].hi, _abi.NODE_INNER, 2 * k + 2
        empty.lo, empty.hi, empty.kind, empty.link = old[0].lo, old[0].lo, _abi.NODE_EMPTY, 0
    for i in range(n):
        nodes[2 * wraps + i] = old[i]
        if old[i].kind == _abi.NODE_INNER:
            nodes[2 * wraps + i].link = old[i].link + 2 * wraps
    sc.wrapped_nodes = nodes      # (the description points into it)
    d.nodes = C.cast(nodes, type(d.nodes))
    d.node_count = n + 2 * wraps
    return sc


def test_a_scene_whose_large_request_does_not_fit(dev, oracle):
    """121 nodes and 16 triangles: the rotated copies fit a quarter of a compute unit's LDS, eight node arrays beside the cold
    words of 1024 lanes do not fit the whole (167 168 bytes)"""
    sc = wrapped(host.lds_edge_scene(16, 2, 0, cases.SEED[16], cases.W, cases.H), 45)
    assert sc.d.node_count == 121
    chosen = cases.choice(sc, dev.SENSOR_FRAME)
    assert chosen[1] == ROTATED and large_request(121, chosen[3]) > 160 * 1024
    ref, _ = oracle.render(sc, cases.S)
    got, small = both_forms(dev, sc, cases.S, expect=SMALL)
    assert ref.any() and bits_differing(got, ref) == 0 and bits_differing(small, ref) == 0


def test_a_tree_with_an_inverted_box(dev, oracle):
    """a leaf's box with lo > hi on one axis has no ordered copies: the launch keeps the workgroups of 256 lanes, whose box test
    sorts the slab distances as the reference's does (to both, the box is the one with the two bounds exchanged)"""
    sc = host.cornell(32, 32, 1, 2)
    nodes = sc.d.nodes
    leaf = [i for i in range(int(sc.d.node_count)) if nodes[i].kind == _abi.NODE_TRIANGLE][5]
    nodes[leaf].lo[1], nodes[leaf].hi[1] = nodes[leaf].hi[1] + 0.25, nodes[leaf].lo[1] - 0.25
    assert nodes[leaf].lo[1] > nodes[leaf].hi[1]
    ref, _ = oracle.render(sc, 2)
    got, small = both_forms(dev, sc, 2, expect=SMALL)
    assert ref.any() and bits_differing(got, ref) == 0 and bits_differing(small, ref) == 0


def test_the_sliced_twin_in_the_large_form(dev, oracle):
    """more pixels than the device has lanes in flight: the pool hands them out in two units to the large form's sliced twin; a
    band of the frame against the oracle, the whole frame against the launch of 256 lanes in one piece"""
    from tests.test_gpu_sliced import H, W
    sc = host.cornell(W, H, 1, 2)
    rows = (H // 2 - 4, 8)
    ref, _ = oracle.render(sc, 2, block=(rows[0] * W, rows[1] * W))
    band = slice(rows[0], rows[0] + rows[1])
    ds = dev.DeviceScene(sc)
    try:
        dev.set_slices(2)
        got, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED + ", sliced x2", LARGE), ran(dev)
        dev.set_slices(1)
        dev.lib().wpt_set_walk(dev.WALK_SMALL_WORKGROUPS)
        whole, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED, SMALL), ran(dev)
    finally:
        dev.set_slices(0)
        dev.lib().wpt_set_walk(0)
        ds.close()
    assert ref[band].any() and bits_differing(got[band], ref[band]) == 0
    assert bits_differing(got, whole) == 0
