"""The transient film on the GPU: one launch renders the frame and K path-length bins, and bin k is bit for bit the oracle's
render gated to [e_k, e_{k+1}) (min_path_len = e_k, max_path_len = nextafterf(e_{k+1}, -inf)), for every kind of scene,
every schedule (pool, two passes, forced wavefront form) and for blocks."""
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import host

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


def gated_params(base, lo, hi):
    """the SensorRGB gate that bin [lo, hi) replaces"""
    p = host.default_params() if base is None else type(base).from_buffer_copy(base)
    p.min_path_len = float(np.float32(lo))
    p.max_path_len = float(np.nextafter(np.float32(hi), np.float32(-np.inf)))
    return p


def check_bins(oracle, sc, s, edges, bins, params=None, block=None, which=None, rows=None):
    """bins[k] == the oracle's gated frame for the bins in `which` (all by default); `rows`: compare these rows only"""
    edges = np.asarray(edges, np.float32)
    for k in (range(len(edges) - 1) if which is None else which):
        ref, _ = oracle.render(sc, s, params=gated_params(params, edges[k], edges[k + 1]), block=block)
        got = bins[k] if rows is None else bins[k][rows]
        ref = ref if rows is None else ref[rows]
        nbad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        assert nbad == 0, "bin %d [%g, %g): %d of %d values differ" % (k, edges[k], edges[k + 1], nbad, got.size)


def test_bins_bit_exact_against_gated_renders(dev, oracle):
    sc = host.cornell(32, 32, 1, 2)
    s = 3
    edges = dev.uniform_edges(0.0, 1.5, 8)
    ds = dev.DeviceScene(sc)
    frame, bins = ds.render_transient(s, edges)
    assert "transient" in dev.lib().wpt_kernel_name().decode()
    assert bins.shape == (8, 32, 32, 3) and np.isfinite(bins).all()
    assert sum(int(bins[k].any()) for k in range(8)) >= 4          # the light arrives over several bins
    check_bins(oracle, sc, s, edges, bins)
    plain, _ = ds.render(s)
    ref, _ = oracle.render(sc, s)
    assert bits_equal(frame, plain) and bits_equal(frame, ref)


def _scenes():
    def lens():
        sc = host.cornell(40, 32, 1, 2)
        host.set_distortion(sc, 3, k1=-0.25, k2=0.09, k3=-0.015, p1=0.0011, p2=-0.0007)
        return sc

    def surround():
        sc = host.cornell(48, 24, 1, 2)
        host.set_camera_mode(sc, 2, 0.0)
        return sc

    def stereo():
        sc = host.cornell(32, 32, 1, 2)
        host.set_camera_mode(sc, 0, 0.065)
        return sc

    def thin_lens():
        return host.random_triangles(300, 4, 40, 32, True, 0.08)

    return {
        "spheres": (lambda: host.spheres(48, 40, 1), None),
        "mis_test": (lambda: host.mis_test(48, 32, True), None),
        "furnace": (lambda: host.furnace(32, 32, 4, slices=16), None),
        "texture_probe": (lambda: host.texture_probe(48, 32, 0), None),
        "sponza_like": (lambda: host.sponza_like(48, 32, detail=0.05, tex_size=32, env_width=64, importance_n=16), None),
        "rgl_scene": (lambda: host.rgl_scene(48, 32, 1), None),
        "animated": (lambda: host.animated(48, 32, 8, 0.0, 1.0), (0.0, 1.0)),
        "lens_distortion": (lens, None),
        "surround": (surround, None),
        "stereo": (stereo, None),
        "thin_lens": (thin_lens, None),
        "dispersive_glass": (lambda: host.cornell(32, 32, 1, 3), None),
    }


@pytest.mark.parametrize("name", list(_scenes()))
def test_every_scene_kind(dev, oracle, name):
    """Two bins, a third and an open last bin [e_3, +inf) (the environment's FLT_MAX path length lands there) for every kind
    of scene the plain render takes; the frame of the launch is the plain render's."""
    make, times = _scenes()[name]
    sc = make()
    if sc.d.envmap.N > 0 and not sc.d.envmap.M:
        sc.set_envmap_tables(*oracle.envmap_tables(sc))     # the oracle takes the importance tables from its caller
    p = host.default_params()
    if times is not None:
        p.t0, p.t1 = times
    s = 2
    edges = np.array([0.5, 3.0, 4.5, 7.0, np.inf], np.float32)
    ds = dev.DeviceScene(sc)
    frame, bins = ds.render_transient(s, edges, params=p)
    assert "transient" in dev.lib().wpt_kernel_name().decode()
    assert bins.any(), "no light in any bin"
    check_bins(oracle, sc, s, edges, bins, params=p)
    ref, _ = oracle.render(sc, s, params=p)
    assert bits_equal(frame, ref)


def test_dispersive_glass_bins_channels_apart(dev, oracle):
    """With a refractive index per channel the channels' optical path lengths differ: a pixel's channels land in different
    bins.  Fine bins over the box, all checked."""
    sc = host.cornell(32, 32, 1, 3)
    s = 3
    edges = dev.uniform_edges(3.0, 0.25, 24)
    frame, bins = dev.DeviceScene(sc).render_transient(s, edges)
    check_bins(oracle, sc, s, edges, bins)
    nonzero = bins > 0
    # somewhere one channel is in a bin that another channel of the same pixel is not in
    assert (nonzero.any(axis=-1) & ~nonzero.all(axis=-1)).any()


def test_block_semantics(dev, oracle):
    import torch
    sc = host.cornell(32, 32, 1, 2)
    w, h, s = 32, 32, 2
    edges = dev.uniform_edges(1.0, 2.0, 5)
    ds = dev.DeviceScene(sc)
    sentinel = -7.25
    frame = torch.full((h, w, 3), sentinel, dtype=torch.float32, device="cuda")
    bins = torch.full((5, h, w, 3), sentinel, dtype=torch.float32, device="cuda")
    start, size = 100, 333
    ds.render_transient_into(frame, bins, s, edges, block=(start, size), stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    f, b = frame.cpu().numpy().reshape(-1, 3), bins.cpu().numpy().reshape(5, -1, 3)
    inside = np.zeros(w * h, bool)
    inside[start:start + size] = True
    assert (f[~inside] == sentinel).all() and (b[:, ~inside] == sentinel).all()
    assert (f[inside] != sentinel).all() and (b[:, inside] != sentinel).all()
    # two blocks together are one whole-frame launch
    whole_frame, whole_bins = ds.render_transient(s, edges)
    frame.fill_(sentinel)
    bins.fill_(sentinel)
    for blk in ((0, 517), (517, w * h - 517)):
        ds.render_transient_into(frame, bins, s, edges, block=blk, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bits_equal(frame.cpu().numpy(), whole_frame) and bits_equal(bins.cpu().numpy(), whole_bins)
    # the synchronous host form (submitBlock semantics) gives the block's values
    rgb, hb = ds.render_transient_host(s, edges, (start, size))
    assert bits_equal(rgb, whole_frame.reshape(-1, 3)[start:start + size])
    assert bits_equal(hb, whole_bins.reshape(5, -1, 3)[:, start:start + size])
    # without a frame: the bins alone
    bins.fill_(sentinel)
    ds.render_transient_into(None, bins, s, edges, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bits_equal(bins.cpu().numpy(), whole_bins)
    check_bins(oracle, sc, s, edges, whole_bins, which=(0, 2))


def test_pool_and_two_pass_schedules(dev, oracle):
    """Frames larger than the lanes in flight: the pixel pool (scene in LDS and all-features kernel) and the two-pass schedule
    (scene from HBM, 64 spp).  The bins equal the oracle's gated frames on a block of rows."""
    edges = np.array([0.0, 3.5, 5.0, np.inf], np.float32)
    w, h, s = 1024, 640, 2
    sc = host.cornell(w, h, 1, 2)
    rows = slice(300, 308)
    block = (300 * w, 8 * w)
    for variant in (0, 0x02):
        dev.lib().wpt_set_launch_config(0, variant)
        try:
            frame, bins = dev.DeviceScene(sc).render_transient(s, edges)
            assert dev.lib().wpt_last_render_passes() == 1
        finally:
            dev.lib().wpt_set_launch_config(0, 0)
        check_bins(oracle, sc, s, edges, bins, block=block, rows=rows)
        ref, _ = oracle.render(sc, s, block=block)
        assert bits_equal(frame[rows], ref[rows])
    w, h, s = 1536, 1024, 8
    sc = host.cornell(w, h, 1, 2)
    dev.lib().wpt_set_launch_config(0, 0x01)
    try:
        frame, bins = dev.DeviceScene(sc).render_transient(s, edges)
        assert dev.lib().wpt_last_render_passes() == 2
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    rows = slice(500, 504)
    block = (500 * w, 4 * w)
    check_bins(oracle, sc, s, edges, bins, block=block, rows=rows)
    ref, _ = oracle.render(sc, s, block=block)
    assert bits_equal(frame[rows], ref[rows])


def test_forced_wavefront_form_still_renders_the_transient_kernel(dev, oracle):
    sc = host.rgl_scene(48, 32, 1)
    s = 2
    edges = np.array([0.5, 3.0, 4.5, np.inf], np.float32)
    dev.lib().wpt_set_wavefront(1, 0, 0, 0)
    try:
        ds = dev.DeviceScene(sc)
        plain, _ = ds.render(s)
        assert dev.lib().wpt_kernel_name().decode() == "wf_trace + wf_shade"
        frame, bins = ds.render_transient(s, edges)
        assert "transient" in dev.lib().wpt_kernel_name().decode()
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    check_bins(oracle, sc, s, edges, bins)
    assert bits_equal(frame, plain)


def test_bins_add_up_to_the_frame(dev):
    """Edges from 0 to +inf cover every contribution: the sum over the bins is the frame up to float32 summation order."""
    sc = host.cornell(32, 32, 1, 2)
    edges = np.concatenate([dev.uniform_edges(0.0, 0.75, 20), [np.inf]]).astype(np.float32)
    frame, bins = dev.DeviceScene(sc).render_transient(3, edges)
    total = bins.astype(np.float64).sum(axis=0)
    assert frame.sum() > 0
    assert np.allclose(total, frame, rtol=2e-5, atol=1e-6), np.abs(total - frame).max()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0          # little-endian
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


def test_light_in_flight_example_equals_the_python_path(dev, tmp_path):
    exe = str(tmp_path / "light_in_flight")
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "light_in_flight.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe],
                   check=True, timeout=600)
    w, h, s, K, start, width = 32, 24, 3, 12, 2.0, 0.5
    r = subprocess.run([exe, str(w), str(h), str(s), str(K), repr(start), repr(width), str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"transient" in r.stdout
    frame, bins = dev.DeviceScene(host.cornell(w, h, 1, 2)).render_transient(s, dev.uniform_edges(start, width, K))
    assert bins[:, :, :, :].any()
    assert bits_equal(read_pfm(str(tmp_path / "frame.pfm")), frame)
    for k in range(K):
        assert bits_equal(read_pfm(str(tmp_path / ("slice_%03d.pfm" % k))), bins[k]), k
