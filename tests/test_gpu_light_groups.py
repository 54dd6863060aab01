"""Light groups on the GPU: one launch renders the frame and a plane per group of emitters, and plane g is bit for bit the plain
device render of the muted twin for g -- the same description in which only group g's emitters emit -- on each of the four
transient kernels, behind both gates, for blocks, for the pooled and the two-pass launch forms, and through the C++ sensor.
32 x 24 at 9 samples per pixel with max_path_components = 8 unless a test says otherwise."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import light_groups_cases as cases
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = _abi.LIGHT_GROUP_NONE
S = cases.S


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def differing(a, b):
    """how many values differ in their bits"""
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _device():
    from wurblpt_amd import device
    return device


@functools.lru_cache(maxsize=None)
def twin_frame(name, keep, w=cases.W, h=cases.H, s=S, gates=()):
    """the plain device render of the muted twin that keeps the sources in `keep`, computed once"""
    frame, _ = _device().DeviceScene(cases.twin(name, keep, w, h)).render(s, params=cases.params(name, **dict(gates)))
    frame.setflags(write=False)
    return frame


@functools.lru_cache(maxsize=None)
def one_group_each(name):
    """(frame, planes, sources, kernel name) of the launch that gives every source of the scene a group of its own"""
    dev = _device()
    sc = cases.make(name)
    srcs = cases.sources(sc)
    t, env = cases.table(sc, [[s] for s in srcs])
    frame, planes = dev.DeviceScene(sc).render_light_groups(S, t, len(srcs), env, params=cases.params(name))
    kernel = dev.lib().wpt_kernel_name().decode()
    frame.setflags(write=False)
    planes.setflags(write=False)
    return frame, planes, srcs, kernel


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_each_plane_is_its_muted_twins_frame(dev, name):
    """contract 3, K = the number of emitters (plus one for the environment where there is one), all pixels; variants 0 to 3 run
    the four transient kernels, and the kernel that ran is the transient row that wpt_kernel_choice names"""
    frame, planes, srcs, kernel = one_group_each(name)
    sc = cases.make(name)
    d = sc.d
    chosen = dev.kernel_choice(cases.need(sc, cases.params(name)), dev.SENSOR_TRANSIENT, False, d.node_count, d.tri_count, d.material_count)
    assert kernel == chosen[0] and "transient" in kernel
    if name in cases.KERNEL_OF:
        assert kernel == cases.KERNEL_OF[name]
    assert planes.shape == (len(srcs), cases.H, cases.W, 3) and len(srcs) >= 2
    for g, src in enumerate(srcs):
        ref = twin_frame(name, (src,))
        assert np.isfinite(ref).all() and (ref > 0).any(), src
        n = differing(planes[g], ref)
        assert n == 0, "%s, plane %d (source %s): %d of %d values differ from the twin's frame" % (name, g, src, n, ref.size)
    plain, _ = dev.DeviceScene(sc).render(S, params=cases.params(name))
    assert differing(frame, plain) == 0                                                  # contract 1


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_planes_add_up_to_the_frame(dev, name):
    """the planes, summed in float64, against the frame within 2 (m + 1) u * frame, m = 2 * 8 * 9: 1.7e-5 relative"""
    frame, planes, _, _ = one_group_each(name)
    assert (frame > 0).any()
    cases.check_sum(planes, frame, cases.sum_bound(cases.MAX_PATH, S))


def test_one_group_is_the_frame_and_shared_and_empty_groups(dev):
    """contracts 1 and 5 on variant 1 (every kind of emitter): with everything in one group plane 0 is the frame; two emitters that
    share a group give the twin that keeps both; a group nobody is in stays 0, and what is in no group reaches the frame only;
    with every emitter muted every plane is 0"""
    name = "variant1"
    sc = cases.make(name)
    srcs = cases.sources(sc)
    ds = dev.DeviceScene(sc)
    p = cases.params(name)
    plain, _ = ds.render(S, params=p)
    t, env = cases.table(sc, [srcs])
    frame, planes = ds.render_light_groups(S, t, 1, env, params=p)
    assert differing(frame, plain) == 0 and differing(planes[0], plain) == 0 and (plain > 0).any()
    # every record in group 0, the records that do not emit as well: their zeros change nothing
    frame, planes = ds.render_light_groups(S, np.zeros(sc.d.material_count, np.uint8), 1, 0, params=p)
    assert differing(planes[0], plain) == 0
    # lamps 0 and 2 share group 1, the environment and lamp 1 share group 3, group 0 and group 2 are empty, the rest is in no group
    t, env = cases.table(sc, [[], [srcs[0], srcs[2]], [], [srcs[1], "env"]])
    frame, planes = ds.render_light_groups(S, t, 4, env, params=p)
    assert differing(frame, plain) == 0
    assert differing(planes[1], twin_frame(name, (srcs[0], srcs[2]))) == 0
    assert differing(planes[3], twin_frame(name, (srcs[1], "env"))) == 0
    assert not planes[0].any() and not planes[2].any()
    assert planes[0].view(np.uint32).max() == 0                                          # +0, not -0
    # nothing in any group: the frame alone
    frame, planes = ds.render_light_groups(S, np.full(sc.d.material_count, NONE, np.uint8), 3, NONE, params=p)
    assert differing(frame, plain) == 0 and planes.view(np.uint32).max() == 0
    # every emitter muted: all planes (and the frame) are 0
    dark = cases.twin(name, [])
    t, env = cases.table(dark, [[s] for s in srcs])
    frame, planes = dev.DeviceScene(dark).render_light_groups(S, t, len(srcs), env, params=p)
    assert planes.view(np.uint32).max() == 0 and not frame.any()


def test_hit_emission_and_light_ray_land_in_one_plane(dev):
    """mis_test: every lamp is a hot spot, so its light arrives by the path's own hits and by light rays, weighted against each
    other; both land in the lamp's plane, which is the twin's frame -- and without hot spots (hits alone) as well"""
    frame, planes, srcs, _ = one_group_each("mis_test")
    assert len(srcs) == 4
    for g, src in enumerate(srcs):
        assert differing(planes[g], twin_frame("mis_test", (src,))) == 0
    # a lamp seen directly shows its emission (4, 4, 4) in its own plane only
    direct = np.all(np.isclose(planes, 4.0, rtol=1e-3), axis=-1)
    assert direct.any() and (direct.sum(axis=0) <= 1).all()
    cold = host.mis_test(cases.W, cases.H, with_hot_spots=False)
    cold_srcs = cases.sources(cold)
    t, env = cases.table(cold, [[s] for s in cold_srcs])
    p = cases.params()
    _, cold_planes = dev.DeviceScene(cold).render_light_groups(S, t, len(cold_srcs), env, params=p)
    for g, src in enumerate(cold_srcs):
        tw = host.mis_test(cases.W, cases.H, with_hot_spots=False)
        host.mute_emitters(tw, [src])
        ref, _ = dev.DeviceScene(tw).render(S, params=p)
        assert differing(cold_planes[g], ref) == 0
    assert not np.array_equal(cold_planes, planes)                                       # the light rays made a difference


def test_both_gates_apply_to_the_planes(dev):
    """distance gate and path-length gate set, on variant 0 with dispersive glass: the channels' path lengths differ, and the
    gate cuts each channel on its own -- in the planes as in the twins' frames (the transient film gates its bins' frame only)"""
    name = "variant0_dispersive"
    gates = (("min_dist_to_light", 0.4), ("max_dist_to_light", 3.2), ("min_path_len", 4.1), ("max_path_len", 6.3))
    sc = cases.make(name)
    srcs = cases.sources(sc)
    p = cases.params(name, **dict(gates))
    t, env = cases.table(sc, [[s] for s in srcs])
    ds = dev.DeviceScene(sc)
    frame, planes = ds.render_light_groups(S, t, len(srcs), env, params=p)
    assert dev.lib().wpt_kernel_name().decode() == cases.KERNEL_OF["variant0"]
    plain, _ = ds.render(S, params=p)
    ungated, _ = ds.render(S, params=cases.params(name))
    assert differing(frame, plain) == 0 and differing(plain, ungated) > 0 and (plain > 0).any()
    for g, src in enumerate(srcs):
        ref = twin_frame(name, (src,), gates=gates)
        assert (ref > 0).any() and differing(planes[g], ref) == 0, src
    assert differing(planes[0], twin_frame(name, (srcs[0],))) > 0                        # the gates cut into the lamp's light
    cases.check_sum(planes, frame, cases.sum_bound(cases.MAX_PATH, S))
    # each gate alone
    for one in (gates[:2], gates[2:]):
        _, planes = ds.render_light_groups(S, t, len(srcs), env, params=cases.params(name, **dict(one)))
        for g, src in enumerate(srcs):
            assert differing(planes[g], twin_frame(name, (src,), gates=one)) == 0, (one, src)


def test_environment_with_importance_sampling(dev):
    """a Sponza-class scene lit by its environment alone, sampled by importance (no hot spot): the environment in group 0 and
    nothing else in any group; the plane is the frame"""
    sc = host.sponza_like(48, 32, detail=0.05, tex_size=32, env_width=64, importance_n=16)
    assert sc.d.envmap.N == 16 and sc.d.hotspot_count == 0 and host.emitters(sc) == []
    p = cases.params()
    ds = dev.DeviceScene(sc)
    frame, planes = ds.render_light_groups(S, np.full(sc.d.material_count, NONE, np.uint8), 2, 0, params=p)
    assert "transient" in dev.lib().wpt_kernel_name().decode()
    plain, _ = ds.render(S, params=p)
    assert (plain > 0).any() and differing(frame, plain) == 0
    assert differing(planes[0], plain) == 0 and planes[1].view(np.uint32).max() == 0


def test_blocks_and_the_synchronous_form(dev):
    """a block that starts and ends inside a row: only its pixels are written, in the frame and in every plane; two blocks are
    one launch; the synchronous form packs the block's pixels plane after plane"""
    import torch
    name = "variant1"
    w, h = cases.W, cases.H
    sc = cases.make(name)
    srcs = cases.sources(sc)
    K = len(srcs)
    t, env = cases.table(sc, [[s] for s in srcs])
    p = cases.params(name)
    ds = dev.DeviceScene(sc)
    whole_frame, whole_planes, _, _ = one_group_each(name)
    sentinel = -7.25
    frame = torch.full((h, w, 3), sentinel, dtype=torch.float32, device="cuda")
    planes = torch.full((K, h, w, 3), sentinel, dtype=torch.float32, device="cuda")
    start, size = 3 * w + 11, 7 * w + 9                                                  # from inside row 3 to inside row 10
    ds.render_light_groups_into(frame, planes, S, t, K, env, block=(start, size), params=p, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    f, b = frame.cpu().numpy().reshape(-1, 3), planes.cpu().numpy().reshape(K, -1, 3)
    inside = np.zeros(w * h, bool)
    inside[start:start + size] = True
    assert (f[~inside] == sentinel).all() and (b[:, ~inside] == sentinel).all()
    assert differing(f[inside], whole_frame.reshape(-1, 3)[inside]) == 0
    assert differing(b[:, inside], whole_planes.reshape(K, -1, 3)[:, inside]) == 0
    for blk in ((0, start), (start + size, w * h - start - size)):
        ds.render_light_groups_into(frame, planes, S, t, K, env, block=blk, params=p, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert differing(frame.cpu().numpy(), whole_frame) == 0 and differing(planes.cpu().numpy(), whole_planes) == 0
    rgb, hp = ds.render_light_groups_host(S, t, K, (start, size), env, params=p)
    assert differing(rgb, whole_frame.reshape(-1, 3)[start:start + size]) == 0
    assert hp.shape == (K, size, 3) and differing(hp, whole_planes.reshape(K, -1, 3)[:, start:start + size]) == 0
    # without a frame: the planes alone
    planes.fill_(sentinel)
    ds.render_light_groups_into(None, planes, S, t, K, env, params=p, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert differing(planes.cpu().numpy(), whole_planes) == 0
    # a table of another scene's length is refused
    L = dev.lib()
    st = L.wpt_render_light_groups_block_device(ds._handle, sc.camera, C.byref(p), C.c_void_p(t.ctypes.data), t.size - 1, K, int(env), w, h, S,
                                                0, w * h, None, C.c_void_p(planes.data_ptr()), None)
    assert st == 1 and "light groups" in L.wpt_last_error().decode() and "materials" in L.wpt_last_error().decode()


def test_the_largest_group_count(dev):
    """K = 255 at 16 x 12: the lamps in the last and the first group, 253 planes between them stay 0"""
    name = "variant0"
    sc = cases.make(name, 16, 12)
    a, b = cases.sources(sc)
    t = np.full(sc.d.material_count, NONE, np.uint8)
    t[a], t[b] = 254, 0
    frame, planes = dev.DeviceScene(sc).render_light_groups(S, t, 255, NONE, params=cases.params(name))
    assert planes.shape == (255, 12, 16, 3)
    assert differing(planes[254], twin_frame(name, (a,), 16, 12)) == 0 and differing(planes[0], twin_frame(name, (b,), 16, 12)) == 0
    assert planes[254].any() and planes[0].any() and planes[1:254].view(np.uint32).max() == 0


def _smallest_block(dev, sc, p, s, want, cu):
    """the smallest number of pixels for which wpt_launch_plan answers `want` for a transient launch of this scene"""
    d = sc.d
    need = cases.need(sc, p)
    lds = dev.kernel_choice(need, dev.SENSOR_TRANSIENT, False, d.node_count, d.tri_count, d.material_count)[3] > 0
    plan = lambda n: dev.launch_plan(dev.SENSOR_TRANSIENT, False, need, lds, n, s, cu)
    lo, hi = 1, 2
    while not want(plan(hi)):
        lo, hi = hi, hi * 2
        assert hi < 1 << 30
    while hi - lo > 1:                                                                   # want(plan(lo)) is false, want(plan(hi)) true
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if want(plan(mid)) else (mid, hi)
    return hi, plan


@pytest.mark.parametrize("form", ["pooled", "two passes"])
def test_launch_forms(dev, form):
    """variant 1 on one frame just large enough for the pixel pool (4 spp), and on one of the smallest size for which
    wpt_launch_plan answers two passes at samples_sqrt = 8 (the size is that function's answer for this device); planes against
    the twins' frames"""
    import torch
    name = "variant1"
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    s = 2 if form == "pooled" else 8
    p = cases.params(name)
    probe = cases.make(name, 16, 16)
    want = (lambda plan: plan["pooled"]) if form == "pooled" else (lambda plan: plan["strategy"] == "two passes")
    pixels, plan = _smallest_block(dev, probe, p, s, want, cu)
    w = 256 if form == "pooled" else 512
    h = -(-pixels // w)
    assert want(plan(w * h)) and not want(plan(w * (h - 1)))
    if form == "two passes":
        assert plan(w * h)["passes"] == 2
    sc = cases.make(name, w, h)
    srcs = cases.sources(sc)
    t, env = cases.table(sc, [[x] for x in srcs])
    frame, planes = dev.DeviceScene(sc).render_light_groups(s, t, len(srcs), env, params=p)
    assert dev.lib().wpt_last_render_passes() == plan(w * h)["passes"]
    assert dev.lib().wpt_kernel_name().decode() == cases.KERNEL_OF[name]
    for g, src in enumerate(srcs):
        ref, _ = dev.DeviceScene(cases.twin(name, [src], w, h)).render(s, params=p)
        assert (ref > 0).any() and differing(planes[g], ref) == 0, (form, src)
    plain, _ = dev.DeviceScene(sc).render(s, params=p)
    assert differing(frame, plain) == 0


def test_device_mix_is_the_host_mix(dev):
    """the rendered planes of variant 1 mixed on the device and on the host: the same bits; so are the transient film's bins"""
    import torch
    _, planes, srcs, _ = one_group_each("variant1")
    rng = np.random.RandomState(7)
    weights = (rng.rand(len(srcs), 3) * 3).astype(np.float32)
    weights[1] = [-0.75, 0.0, np.float32(1e-40)]
    weights[2, 1] = -0.0
    on_host = dev.mix_planes_host(planes, weights)
    on_device = dev.mix_planes(torch.from_numpy(np.array(planes)).cuda(), weights)
    torch.cuda.synchronize()
    assert differing(on_device.cpu().numpy(), on_host) == 0 and (on_host != 0).any() and (on_host < 0).any()
    # all weights 1: the planes' float32 sum in their order, near the frame
    ones = dev.mix_planes(torch.from_numpy(np.array(planes)).cuda(), np.ones(len(srcs), np.float32)).cpu().numpy()
    acc = np.zeros_like(ones)
    for k in range(len(srcs)):
        acc = acc + planes[k]
    assert differing(ones, acc) == 0
    sc = host.cornell(32, 32, 1, 2)
    edges = dev.uniform_edges(0.0, 2.0, 5)
    frame = torch.zeros((32, 32, 3), dtype=torch.float32, device="cuda")
    bins = torch.zeros((5, 32, 32, 3), dtype=torch.float32, device="cuda")
    dev.DeviceScene(sc).render_transient_into(frame, bins, 2, edges, stream=torch.cuda.current_stream())
    w5 = np.array([0.0, 1.0, 0.5, 2.0, -1.0], np.float32)
    mixed = dev.mix_planes(bins, w5)
    torch.cuda.synchronize()
    assert differing(mixed.cpu().numpy(), dev.mix_planes_host(bins.cpu().numpy(), w5)) == 0 and mixed.abs().sum().item() > 0


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0          # little-endian
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


def test_light_mixer_example_checks_itself(dev, tmp_path):
    """examples/light_mixer.cpp through SensorRGBLightGroups and mcpt(): at 64 x 48 its own comparison of every group's frame with
    the render of the muted twin reports 0 differing bits, and its mixes are the host mix of its groups"""
    exe = str(tmp_path / "light_mixer")
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "light_mixer.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, "64", "48", "3", str(tmp_path), "check"], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()[-2000:]
    assert "3 light groups on kernel wpt_pathtrace, transient" in out
    assert "groups against the renders of their muted twins: 0 differing bits" in out
    groups = np.stack([read_pfm(str(tmp_path / ("group_%d.pfm" % g))) for g in range(3)])
    frame = read_pfm(str(tmp_path / "frame.pfm"))
    assert all(g.any() for g in groups) and (frame > 0).any()
    cases.check_sum(groups, frame, cases.sum_bound(128, 3))                              # the example keeps the default path length
    dimmed = dev.mix_planes_host(groups, np.full(3, 0.25, np.float32))
    assert differing(read_pfm(str(tmp_path / "mix_dimmed.pfm")), dimmed) == 0
    evening = dev.mix_planes_host(groups, np.array([1.0, 0.0, 0.33], np.float32))
    assert differing(read_pfm(str(tmp_path / "mix_evening.pfm")), evening) == 0
