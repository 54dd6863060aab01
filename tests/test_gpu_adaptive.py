"""Adaptive sampling on the GPU: with a sample-count map, pixel p is bit for bit the plain render (and the oracle's) at
samples_sqrt = n_p, for every scene kind of the single kernel; pixels with n_p = 0 keep what they held; block forms, the
synchronous form and the cost order change no bit; the moment film is frame^2 at n = 1 and the fp32 sum of e*e behind a
constant emitter, and its variance estimate predicts the error against a converged render."""
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def nan_tensor(h, w):
    import torch
    return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")


def render_into(dev, ds, m, with_moments=True, block=None):
    """frame and moments of an adaptive render into NaN-filled tensors (numpy)"""
    import torch
    h, w = m.shape
    f = nan_tensor(h, w)
    mo = nan_tensor(h, w) if with_moments else None
    ds.render_adaptive_into(f, m, mo, block=block, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    return f.cpu().numpy(), (mo.cpu().numpy() if with_moments else None)


SCENES = {
    # name: (scene, params t0 t1, launch variant, words of the kernel name, n of the constant map)
    "cornell_lds": (lambda: host.cornell(37, 23, 1, 2), None, 0, "adaptive, scene in LDS", 3),
    "cornell_lds_tiled": (lambda: host.cornell(40, 24, 1, 2), None, 0, "adaptive, scene in LDS", 2),
    "basic_hbm": (lambda: host.cornell(37, 23, 1, 2), None, 0x01, "adaptive, basic", 3),
    "cornell_all_features": (lambda: host.cornell(37, 23, 1, 3), None, 0x02, "adaptive, all features", 2),
    "sponza_like": (lambda: host.sponza_like(37, 23, detail=0.05, tex_size=32, env_width=64, importance_n=16), None, 0,
                    "adaptive, all features", 2),
    "spheres": (lambda: host.spheres(37, 23, 1), None, 0, "adaptive, all features", 2),
    "animated": (lambda: host.animated(37, 23, 8, 0.0, 1.0), (0.0, 1.0), 0, "adaptive, all features, moving scenes", 2),
    "rgl_scene": (lambda: host.rgl_scene(37, 23, 1), None, 0, "adaptive, measured BRDFs", 2),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_constant_map_equals_plain_render_and_oracle(dev, oracle, name):
    import torch
    make, times, variant, words, n = SCENES[name]
    sc = make()
    if sc.d.envmap.N > 0 and not sc.d.envmap.M:
        sc.set_envmap_tables(*oracle.envmap_tables(sc))
    p = host.default_params()
    if times is not None:
        p.t0, p.t1 = times
    m = torch.full((sc.height, sc.width), n, dtype=torch.int32)
    dev.lib().wpt_set_launch_config(0, variant)
    try:
        ds = dev.DeviceScene(sc)
        frame, moments = ds.render_adaptive(m, with_moments=True, params=p)
        name_k = dev.lib().wpt_kernel_name().decode()
        assert words in name_k, name_k
        assert dev.lib().wpt_last_render_passes() == 1
        bare = ds.render_adaptive(m.to(torch.int16), params=p)           # any integer type; no moment film
        plain, _ = ds.render(n, params=p)
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    frame, moments, bare = frame.cpu().numpy(), moments.cpu().numpy(), bare.cpu().numpy()
    assert np.isfinite(frame).all() and frame.any()
    assert bits_equal(frame, plain), "%d values differ from the plain render" % int((frame.view(np.uint32) != plain.view(np.uint32)).sum())
    assert bits_equal(bare, frame), "asking for moments changed the frame"
    ref, _ = oracle.render(sc, n, params=p)
    assert bits_equal(frame, ref), "%d values differ from the oracle" % int((frame.view(np.uint32) != ref.view(np.uint32)).sum())
    # the moment of a mean is at least its square (up to rounding), wherever light arrived
    assert (moments >= 0.0).all() and (moments >= 0.999 * frame * frame).all()


def plain_by_count(dev, ds, counts, p=None):
    return {int(c): ds.render(int(c), params=p)[0] for c in counts if c > 0}


@pytest.mark.parametrize("w,h,variant", [(37, 23, 0), (40, 24, 0), (40, 24, 0x01), (37, 23, 0x02), (40, 24, 0x02)])
def test_random_map_pixels_equal_plain_renders_and_zeros_are_not_written(dev, w, h, variant):
    values = np.array([0, 1, 2, 3, 5, 8])
    rng = np.random.default_rng(1000 + w + variant)
    m = values[rng.integers(0, len(values), (h, w))]
    sc = host.cornell(w, h, 1, 2)
    dev.lib().wpt_set_launch_config(0, variant)
    try:
        ds = dev.DeviceScene(sc)
        frame, moments = render_into(dev, ds, m)
        plain = plain_by_count(dev, ds, values)
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    zero = m == 0
    assert np.isnan(frame[zero]).all() and np.isnan(moments[zero]).all()
    assert np.isfinite(frame[~zero]).all() and np.isfinite(moments[~zero]).all()
    for n, ref in plain.items():
        sel = m == n
        assert sel.any()
        assert bits_equal(frame[sel], ref[sel]), "n = %d: %d values differ" % (n, int((frame[sel].view(np.uint32) != ref[sel].view(np.uint32)).sum()))
    assert bits_equal(moments[m == 1], frame[m == 1] * frame[m == 1])


def test_block_forms_and_host_form_equal_the_full_frame(dev):
    import torch
    w, h = 37, 23
    rng = np.random.default_rng(7)
    m = np.array([0, 1, 2, 4])[rng.integers(0, 4, (h, w))]
    sc = host.cornell(w, h, 1, 2)
    ds = dev.DeviceScene(sc)
    full_f, full_m = render_into(dev, ds, m)
    # three device blocks into one NaN frame
    f = nan_tensor(h, w)
    mo = nan_tensor(h, w)
    for blk in ((0, 100), (100, 333), (433, w * h - 433)):
        ds.render_adaptive_into(f, torch.as_tensor(m), mo, block=blk, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    assert bits_equal(f.cpu().numpy(), full_f) and bits_equal(mo.cpu().numpy(), full_m)
    # a block alone writes nothing outside it
    one_f, one_m = render_into(dev, ds, m, block=(200, 150))
    inside = np.zeros(w * h, bool)
    inside[200:350] = True
    inside = inside.reshape(h, w)
    assert np.isnan(one_f[~inside]).all() and np.isnan(one_m[~inside]).all()
    assert bits_equal(one_f[inside], full_f[inside]) and bits_equal(one_m[inside], full_m[inside])
    # the synchronous host form: submitBlock semantics, pixels with n = 0 keep the caller's values
    start, size = 123, 456
    rgb = np.full((size, 3), 7.5, np.float32)
    mom = np.full((size, 3), -2.5, np.float32)
    ds.render_adaptive_host(m, (start, size), rgb, mom)
    zero = m.reshape(-1)[start:start + size] == 0
    assert (rgb[zero] == 7.5).all() and (mom[zero] == -2.5).all()
    assert bits_equal(rgb[~zero], full_f.reshape(-1, 3)[start:start + size][~zero])
    assert bits_equal(mom[~zero], full_m.reshape(-1, 3)[start:start + size][~zero])
    rgb2 = np.zeros((size, 3), np.float32)
    ds.render_adaptive_host(m, (start, size), rgb2)                        # without moments: the same frame
    assert bits_equal(rgb2[~zero], rgb[~zero])


@pytest.mark.parametrize("variant", [0, 0x01, 0x02])
def test_cost_order_changes_no_bit(dev, variant):
    """1024 x 512 = 524 288 pixels: twice the lanes that are resident at once in these kernels (256 CUs x 4 workgroups of 256
    lanes), so the launch keeps its pixel pool and the ordered pass hands `order` out through it.  A few 8x8 tiles at n = 8 and
    the rest at n = 1.  The cost order (default) and the plain order (variant bit 0x40) give the same bits, and those of the
    plain renders."""
    w, h = 1024, 512
    m = np.full((h, w), 1, np.int32)
    rng = np.random.default_rng(11)
    for _ in range(24):
        ty, tx = rng.integers(0, h // 8), rng.integers(0, w // 8)
        m[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = 8
    sc = host.cornell(w, h, 1, 2)
    out = {}
    try:
        for order_off in (0, 0x40):
            dev.lib().wpt_set_launch_config(0, variant | order_off)
            ds = dev.DeviceScene(sc)
            out[order_off] = render_into(dev, ds, m)
        dev.lib().wpt_set_launch_config(0, variant)
        plain = plain_by_count(dev, ds, [1, 8])
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    assert bits_equal(out[0][0], out[0x40][0]) and bits_equal(out[0][1], out[0x40][1])
    for n, ref in plain.items():
        assert bits_equal(out[0][0][m == n], ref[m == n]), "n = %d" % n


def test_moments_at_one_sample_are_frame_squared(dev):
    import torch
    for sc in (host.cornell(64, 48, 1, 3), host.sponza_like(37, 23, detail=0.05, tex_size=32, env_width=64, importance_n=16)):
        ds = dev.DeviceScene(sc)
        frame, moments = ds.render_adaptive(torch.ones((sc.height, sc.width), dtype=torch.int64), with_moments=True)
        frame, moments = frame.cpu().numpy(), moments.cpu().numpy()
        assert frame.any()
        assert bits_equal(moments, frame * frame)


def test_constant_emitter_moment_is_the_sum_of_e_squared(dev):
    """Camera rays that end on the diffuse light add the same e in every sample and nothing else: their moment is
    invSamples * (fp32 sum of e*e, sample by sample)"""
    import torch
    w, h, n = 96, 96, 4
    sc = host.cornell(w, h, 0, 0)
    ds = dev.DeviceScene(sc)
    lights = [i for i in range(sc.d.material_count) if sc.d.materials[i].type == _abi.MAT_LIGHT_DIFFUSE]
    assert len(lights) == 1
    e = np.array(list(sc.d.materials[lights[0]].v[0])[:3], np.float32)     # LightDiffuse's emission, untextured
    frame, moments = ds.render_adaptive(torch.full((h, w), n, dtype=torch.int32), with_moments=True)
    frame, moments = frame.cpu().numpy(), moments.cpu().numpy()
    N = n * n
    inv = np.float32(1.0) / np.float32(N)
    acc = np.zeros(3, np.float32)
    mom = np.zeros(3, np.float32)
    for _ in range(N):
        acc = (acc + e).astype(np.float32)
        mom = (mom + (e * e).astype(np.float32)).astype(np.float32)
    want_f = (inv * acc).astype(np.float32)
    want_m = (inv * mom).astype(np.float32)
    sel = (frame == want_f).all(axis=2)
    assert sel.sum() >= 4, "no pixel sees only the light"
    assert (moments[sel] == want_m).all()
    # and their estimated variance is zero
    assert (moments[sel] - frame[sel] * frame[sel] <= 1e-6 * want_m).all()


def test_variance_estimate_predicts_the_error(dev):
    """Lambertian Cornell box (no glass, no GGX: no fireflies), 64 x 64 pixels.  The n = 4 render's squared error against a
    32^2-spp plain render, over the mean predicted variance of the mean from its moments (var * N / (N - 1) / N)."""
    import torch
    w, h, n = 64, 64, 4
    sc = host.cornell(w, h, 0, 0)
    ds = dev.DeviceScene(sc)
    frame, moments = ds.render_adaptive(torch.full((h, w), n, dtype=torch.int32), with_moments=True)
    f = frame.cpu().numpy().astype(np.float64)
    mo = moments.cpu().numpy().astype(np.float64)
    N = n * n
    pred = np.maximum(mo - f * f, 0.0) * N / (N - 1) / N
    ratios = {}
    for ref_sqrt in (32, 64):
        ref = ds.render(ref_sqrt)[0].astype(np.float64)
        ratios[ref_sqrt] = float(np.mean((f - ref) ** 2) / np.mean(pred))
    print("calibration: mse / predicted variance = %.4f (32^2 spp reference), %.4f (64^2 spp reference)" % (ratios[32], ratios[64]))
    # Measured on the first GPU run: 0.4640 against the 32^2-spp reference, 0.4728 against 64^2 spp.  Stratified jitter makes
    # the error of the n = 4 mean about half of what the i.i.d. estimate predicts.  The two references differ in two effects
    # that push in opposite directions: the 32^2 reference's own variance, larger, raises the observed error, and its
    # correlation with the n = 4 render through the shared generator, also larger, lowers it.  So the 2 % between 0.4640 and
    # 0.4728 is a lower bound on what the correlation takes off, not its size.  The render is deterministic: the ratio is the
    # same every run.
    assert ratios[32] <= 1.25
    assert ratios[32] >= 0.40


def test_adaptive_example_runs_and_writes_its_outputs(tmp_path):
    exe = str(tmp_path / "adaptive")
    subprocess.run(["g++", "-std=c++20", "-O2", "-fopenmp", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "adaptive.cpp"),
                    "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, "128", "128", "4", "0.1", "16", str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"adaptively" in r.stdout and b"adaptive" in r.stdout
    for name in ("adaptive.png", "adaptive-map.png"):
        assert os.path.getsize(str(tmp_path / name)) > 100


def test_launch_on_another_stream_sees_the_map(dev):
    """The map is made into 16-bit words on torch's current stream and the launch runs on the caller's stream: the launch
    stream must wait for it.  A launch on a second (non-blocking) stream, and one with stream=None inside `with
    torch.cuda.stream(...)`, give the current-stream result bit for bit, for a host map, a CUDA int64 map and a CUDA uint16 map."""
    import torch
    w, h = 64, 48
    rng = np.random.default_rng(21)
    m = np.array([0, 1, 2, 3])[rng.integers(0, 4, (h, w))]
    sc = host.cornell(w, h, 1, 2)
    ds = dev.DeviceScene(sc)
    want_f, want_m = render_into(dev, ds, m)
    side = torch.cuda.Stream()
    maps = {
        "host int64": lambda: m,
        "cuda int64": lambda: torch.as_tensor(m, device="cuda") * 1,           # written by a kernel on the current stream
        "cuda uint16": lambda: (torch.as_tensor(m, device="cuda") * 1).to(torch.int16).view(torch.uint16),
    }
    for name, make in maps.items():
        for how in ("stream=side", "inside side"):
            torch.cuda.synchronize()
            # a long kernel on the current stream first, so that a launch that does not wait for it would run ahead
            big = torch.randn(4096, 4096, device="cuda")
            for _ in range(8):
                big = big @ big / 64.0
            f, mo = nan_tensor(h, w), nan_tensor(h, w)
            mp = make()
            if how == "stream=side":
                ds.render_adaptive_into(f, mp, mo, stream=side)
            else:
                with torch.cuda.stream(side):
                    side.wait_stream(torch.cuda.default_stream())
                    ds.render_adaptive_into(f, mp, mo)
            torch.cuda.synchronize()
            ds.check()
            assert bits_equal(f.cpu().numpy(), want_f) and bits_equal(mo.cpu().numpy(), want_m), (name, how)


def test_cuda_maps_are_checked_on_the_device(dev):
    import torch
    sc = host.cornell(16, 8, 1, 2)
    ds = dev.DeviceScene(sc)
    f = nan_tensor(8, 16)
    with pytest.raises(ValueError):
        ds.render_adaptive_into(f, torch.full((8, 16), 65536, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ds.render_adaptive_into(f, torch.full((8, 16), -1, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        ds.render_adaptive_into(f, torch.full((8, 16), 2.0, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isnan(f).all()                                             # nothing was launched
