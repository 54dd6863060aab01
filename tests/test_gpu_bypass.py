"""The kernels with the scene in LDS leave inner nodes out of their walk whose children's boxes lie within their own
(wurblpt_amd/csrc/wpt_bypass.h); wpt_set_walk(WPT_WALK_NO_BYPASS) keeps the folded tree, WPT_WALK_NO_FOLD the plain one, and
wpt_set_bypass(1) leaves out every eligible node instead of the cost model's choice.  The leaves tested, their order and every
bound are the same, so every launch renders the same frame bit for bit in all four: the plain kernel and its rotated and sliced
twins, rays whose box tests take the NaN form (they keep the exact links), a tree with a box that is not nested, and the
transient, time-of-flight, views and adaptive kernels.  The Cornell frames are the oracle's as well."""
import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu


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


def modes(dev, sc, launch, walk=0):
    """what `launch(scene)` returns with the model's plan, with every eligible node left out, under NO_BYPASS and under NO_FOLD"""
    out = []
    try:
        ds = dev.DeviceScene(sc)
        dev.set_bypass(dev.BYPASS_ALL_ELIGIBLE)
        ds_all = dev.DeviceScene(sc)
        dev.set_bypass(dev.BYPASS_MODEL)
        assert ds_all.bypassed_nodes() >= ds.bypassed_nodes()
        for scene, flags in ((ds, walk), (ds_all, walk), (ds, walk | dev.WALK_NO_BYPASS), (ds, walk | dev.WALK_NO_FOLD)):
            dev.lib().wpt_set_walk(flags)
            out.append(launch(scene))
    finally:
        dev.set_bypass(dev.BYPASS_MODEL)
        dev.lib().wpt_set_walk(0)
    return out, ds.bypassed_nodes(), ds_all.bypassed_nodes()


@pytest.mark.parametrize("tall,short", [(1, 2), (0, 0)])
def test_cornell_frames_in_all_four_modes_are_the_oracles(dev, oracle, tall, short):
    sc = host.cornell(64, 64, tall, short)
    ref, _ = oracle.render(sc, 4)
    for walk in (0, dev.WALK_SELECT_CORNERS):                   # the rotated form and the form that selects the corners
        frames, model, everything = modes(dev, sc, lambda ds: ds.render(4)[0], walk)
        assert 0 < model == dev.bypass_plan(sc) < everything
        for frame in frames:
            assert bits_differing(frame, ref) == 0


def test_rays_whose_box_tests_take_the_nan_form(dev, oracle):
    """Pixel centres of an odd-sized frame seen along an axis: direction components of exactly zero, slab distances 0 * inf;
    those rays keep the exact links."""
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    for sc in (host.random_triangles(100, 7, 33, 33, with_texcoords=False), host.cornell(33, 33, 1, 2)):
        assert sc.d.node_count * 32 + sc.d.tri_count * 48 <= 20 * 1024
        root = sc.d.nodes[0]
        lo, hi = np.array(root.lo[:], np.float64), np.array(root.hi[:], np.float64)
        mid = 0.5 * (lo + hi)
        saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
        try:
            for axis, sign in ((0, 1.0), (1, -1.0), (2, -1.0)):
                d = np.zeros(3)
                d[axis] = sign
                sc.camera[0] = host.camera_looking_at(sc, mid, mid + d, (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0))
                frames, _, everything = modes(dev, sc, lambda ds: ds.render(2, params=p)[0])
                assert everything > 0
                ref, _ = oracle.render(sc, 2, p)
                for frame in frames:
                    assert bits_differing(frame, ref) == 0, (sc.name, axis)
        finally:
            sc.camera[0] = saved


def test_a_tree_with_a_box_that_is_not_nested(dev, oracle):
    """Child boxes grown beyond their parent's, and one with lo > hi whose bounds as stored lie within the parent's but which
    the box test takes for a box far outside it (a tree handed in through the C ABI need not be nested): those parents stay in
    the walk even when every eligible node is left out -- a link still leads to each of them."""
    sc = host.random_triangles(40, 3, 32, 32, with_texcoords=False)
    nodes = sc.d.nodes
    inner = [i for i in range(int(sc.d.node_count)) if nodes[i].kind == 0]
    try:
        dev.set_bypass(dev.BYPASS_ALL_ELIGIBLE)
        count, links, start = dev.bypass_plan(sc, with_words=True)
        assert count > 3 and start != 0
        parents = [i for i in inner[1:] if not (links[:, 0] == i).any() and not (links[:, 1] == i).any()][:4]   # left out while nested
        assert len(parents) == 4
        for i in parents[:3]:
            nodes[i + 1].hi[0] = nodes[i].hi[0] + 0.25
            nodes[i + 1].lo[1] = nodes[i].lo[1] - 0.25
        i = parents[3]
        nodes[i + 1].lo[2] = 0.5 * (nodes[i].lo[2] + nodes[i].hi[2])
        nodes[i + 1].hi[2] = nodes[i].lo[2] - 5.0           # hi <= the parent's hi, lo >= its lo: the slab is [lo.z - 5, middle]
        assert nodes[i + 1].lo[2] >= nodes[i].lo[2] and nodes[i + 1].hi[2] <= nodes[i].hi[2]
        count2, links, start = dev.bypass_plan(sc, with_words=True)
        assert count2 <= count - 4
        for i in parents:
            assert start == i or (links[:, 0] == i).any() or (links[:, 1] == i).any(), i
    finally:
        dev.set_bypass(dev.BYPASS_MODEL)
    ref, _ = oracle.render(sc, 3)
    frames, _, _ = modes(dev, sc, lambda ds: ds.render(3)[0])
    for frame in frames:
        assert bits_differing(frame, ref) == 0


def test_a_pooled_sliced_launch(dev):
    """more pixels than the device has lanes in flight: the pool hands them out, in two units of one row of strata each"""
    sc = host.cornell(640, 512, 1, 2)
    try:
        dev.set_slices(2)
        forms = []

        def launch(ds):
            frame = ds.render(2)[0]
            forms.append(dev.lib().wpt_kernel_form().decode())
            return frame
        frames, _, _ = modes(dev, sc, launch)
        frames += modes(dev, sc, launch, dev.WALK_SELECT_CORNERS)[0]      # the sliced twin of the form that selects the corners
    finally:
        dev.set_slices(0)
    assert forms == ["rotated corners, sliced x2"] * 4 + [", sliced x2"] * 4   # (wpt_kernel_form: the form, then ", sliced xU")
    assert frames[0].any()
    for frame in frames[1:]:
        assert bits_differing(frames[0], frame) == 0


def test_transient_tof_views_and_adaptive_launches(dev):
    sc = host.cornell(64, 64, 1, 2)
    edges = dev.uniform_edges(0.0, 1.0, 8)
    names = []

    def named(launch):
        def run(ds):
            got = launch(ds)
            names.append(dev.lib().wpt_kernel_name().decode())
            return got
        return run

    def transient(ds):
        frame, bins = ds.render_transient(3, edges)
        return np.concatenate([frame[None], bins])

    sensor = host.tof_sensor(contrast=0.75)
    cams = [_abi.Camera.from_buffer_copy(sc.camera.contents),
            host.camera_looking_at(sc, (0.3, 1.2, 2.9), (0.0, 0.9, 0.0))]
    counts = (np.arange(64 * 64, dtype=np.int64).reshape(64, 64) % 5).astype(np.uint16)   # 0 .. 4 rows of strata per pixel

    def adaptive(ds):
        frame, moments = ds.render_adaptive(counts, with_moments=True)
        return np.stack([frame.cpu().numpy(), moments.cpu().numpy()])

    for launch, name in ((transient, "wpt_pathtrace, transient, scene in LDS"),
                         (lambda ds: ds.render_tof(3, sensor), "wpt_pathtrace, time of flight, scene in LDS"),
                         (lambda ds: ds.render_views(3, cams).cpu().numpy(), "wpt_pathtrace, views, scene in LDS"),
                         (adaptive, "wpt_pathtrace, adaptive, scene in LDS")):
        del names[:]
        frames, _, _ = modes(dev, sc, named(launch))
        assert names == [name] * 4
        assert np.asarray(frames[0]).any()
        for frame in frames[1:]:
            assert bits_differing(frames[0], frame) == 0, name
