"""The kernels with rotated corner copies run a leaf pass in one LDS round trip: the node step keeps the leaf's word, which
says where the triangle's corners lie, and the corner records carry the leaf's skip links and the triangle's index
(wurblpt_amd/csrc/wpt_leaf_words.h).  Every frame here is the oracle's bit for bit: the Cornell box through the product path
and its twins, rays whose box tests take the NaN form (the leaf pass then takes the exact skip link from the record), the
scenes on either side of the edge where the rotated copies stop fitting, and a tree in which a triangle has two leaves and
another none, which keeps the leaf pass that reads the leaf's node (wpt_kernel_form says so)."""
import numpy as np
import pytest

from wurblpt_amd import _abi, host

from tests import lds_edge_cases as cases

pytestmark = pytest.mark.gpu

ROTATED = "rotated corners"
FROM_NODES = "rotated corners, leaf links from the nodes"


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
    return dev.lib().wpt_kernel_name().decode(), dev.lib().wpt_kernel_form().decode()


def test_cornell_through_the_product_path(dev, oracle):
    """64 x 64 at 16 spp: fewer pixels than the device has lanes, so the launch has no pool and runs the kernel that is not
    sliced -- with the pool switched off as well, and under every set of links"""
    sc = host.cornell(64, 64, 1, 2)
    ref, _ = oracle.render(sc, 4)
    ds = dev.DeviceScene(sc)
    try:
        for variant, flags in ((0, 0), (0x40, 0), (0, dev.WALK_NO_BYPASS), (0, dev.WALK_NO_FOLD)):
            dev.lib().wpt_set_launch_config(0, variant)
            dev.lib().wpt_set_walk(flags)
            got, _ = ds.render(4)
            assert ran(dev) == ("wpt_pathtrace", ROTATED), (variant, flags, ran(dev))
            differing = bits_differing(got, ref)
            print("variant %#x walk %d: %d differing bits" % (variant, flags, differing))
            assert differing == 0, (variant, flags)
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
        dev.lib().wpt_set_walk(0)
        ds.close()


def test_the_sliced_twin(dev, oracle):
    """more pixels than the device has lanes in flight: the pool hands them out in two units, the twin that is built from
    wpt_k_basic_lds_rot_sliced.hip; a band of the frame against the oracle, the whole frame against the launch in one piece"""
    from tests.test_gpu_sliced import H, W
    sc = host.cornell(W, H, 1, 2)
    rows = (H // 2 - 4, 8)
    ref, _ = oracle.render(sc, 2, block=(rows[0] * W, rows[1] * W))
    band = slice(rows[0], rows[0] + rows[1])
    ds = dev.DeviceScene(sc)
    try:
        dev.set_slices(1)
        whole, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED)
        dev.set_slices(2)
        got, _ = ds.render(2)
        assert ran(dev) == ("wpt_pathtrace", ROTATED + ", sliced x2")
    finally:
        dev.set_slices(0)
        ds.close()
    assert ref[band].any() and bits_differing(got[band], ref[band]) == 0
    assert bits_differing(got, whole) == 0


@pytest.mark.parametrize("size", [32, 33])
def test_rays_that_take_the_nan_group_in_a_leaf_pass(dev, oracle, size):
    """Rays through the pixels' centres from a camera that looks down an axis.  In the odd-sized frame the centre column and row
    have a direction component of exactly zero: slab distances 0 * inf, RAY_MAY_NAN, and every lane of such a ray's group walks
    the exact links and takes the exact skip link from the corner record.  (The even-sized frame has no pixel on the axes.)"""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    sc = host.cornell(size, size, 1, 2)
    root = sc.d.nodes[0]
    mid = 0.5 * (np.array(root.lo[:], np.float64) + np.array(root.hi[:], np.float64))
    saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
    ds = dev.DeviceScene(sc)
    try:
        for axis, sign in ((0, 1.0), (1, -1.0), (2, -1.0)):
            d = np.zeros(3)
            d[axis] = sign
            sc.camera[0] = host.camera_looking_at(sc, mid, mid + d, (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0))
            ref, _ = oracle.render(sc, 2, p)
            for flags in (0, dev.WALK_NO_BYPASS):
                dev.lib().wpt_set_walk(flags)
                got, _ = ds.render(2, params=p)
                assert ran(dev) == ("wpt_pathtrace", ROTATED)
                differing = bits_differing(got, ref)
                print("axis %d walk %d: %d differing bits" % (axis, flags, differing))
                assert ref.any() and differing == 0, (axis, flags)
    finally:
        dev.lib().wpt_set_walk(0)
        sc.camera[0] = saved
        ds.close()


@pytest.mark.parametrize("t,m", [(36, 2), (37, 2)])
def test_the_capacity_edge_of_the_rotated_copies(dev, oracle, t, m):
    """the largest tree of triangles whose rotated copies fit and the smallest whose copies do not (tests/lds_edge_cases.py)"""
    sc = cases.scene(t, m, 0, 16, 16)
    chosen = cases.choice(sc, dev.SENSOR_FRAME)
    assert cases.side(sc, chosen) == cases.PLAIN[(t, m)]
    assert (chosen[1] == ROTATED) == (t == 36)
    ref, _ = oracle.render(sc, 2)
    ds = dev.DeviceScene(sc)
    try:
        got, _ = ds.render(2)
        assert ran(dev) == (chosen[0], chosen[1])
    finally:
        ds.close()
    differing = bits_differing(got, ref)
    print("%d triangles: %s, %d differing bits" % (t, chosen[1] or "select form", differing))
    assert ref.any() and differing == 0


def test_a_tree_that_is_not_one_leaf_per_triangle(dev, oracle):
    """Through the C ABI a leaf may name any triangle: one leaf is made to name the triangle of another, so that triangle
    has two leaves and the first leaf's own has none.  The oracle walks the same description.  The scene still gets the rotated
    kernel, whose leaf pass then reads the skip links from the leaf's node -- the exact ones too, for the rays through the pixels'
    centres of an odd-sized frame seen along an axis."""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    for size, params, label in ((32, None, "random rays"), (33, p, "rays through the pixels' centres")):
        sc = host.cornell(size, size, 1, 2)
        nodes = sc.d.nodes
        lights = {i for i in range(int(sc.d.material_count)) if sc.d.materials[i].type == _abi.MAT_LIGHT_DIFFUSE}
        leaves = [i for i in range(int(sc.d.node_count)) if nodes[i].kind == 1 and sc.d.tri_geom[nodes[i].link].material not in lights]
        a, b = leaves[len(leaves) // 2], leaves[len(leaves) // 2 + 3]
        assert nodes[a].link != nodes[b].link
        nodes[a].link = nodes[b].link
        untouched = host.cornell(size, size, 1, 2)
        if params is not None:
            root = nodes[0]
            mid = 0.5 * (np.array(root.lo[:], np.float64) + np.array(root.hi[:], np.float64))
            for scene in (sc, untouched):
                scene.camera[0] = host.camera_looking_at(scene, mid, mid + np.array([0.0, 0.0, -1.0]))
        ref, _ = oracle.render(sc, 2, params)
        plain, _ = oracle.render(untouched, 2, params)
        assert bits_differing(ref, plain) > 0, "the changed leaf shows in no pixel"
        ds = dev.DeviceScene(sc)
        try:
            for flags in (0, dev.WALK_NO_BYPASS, dev.WALK_NO_FOLD):
                dev.lib().wpt_set_walk(flags)
                got, _ = ds.render(2, params=params)
                assert ran(dev) == ("wpt_pathtrace", FROM_NODES), ran(dev)
                differing = bits_differing(got, ref)
                print("%s, walk %d: %d differing bits" % (label, flags, differing))
                assert differing == 0, (label, flags)
        finally:
            dev.lib().wpt_set_walk(0)
            ds.close()
