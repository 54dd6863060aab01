"""The rolling shutter on the device (wpt_render_shutter_*): row r of a rolling frame is bit for bit row r of the plain render
with row r's interval, on the device and in the CPU restatement.  Every case renders 32 x 24 pixels at 3^2 samples from one
host.animated scene, bounded for the whole readout and uploaded once; all comparisons are on uint32 views, with 0 differing
values."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import shutter_cases as cases
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H, S = cases.W, cases.H, cases.S
ROW_TIME = F32(0.75) / F32(23)  # with t1 - t0 = 0.25 the readout spans [0, 1]: tests/test_shutter.py shows that it rolls


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from wurblpt_amd import device
    assert device.device_count() >= 1
    return device


def differing(a, b):
    return int((cases.bits(a) != cases.bits(b)).sum())


def rolling_scene(dev, variant, shutter, t0, t1):
    first, last = dev.shutter_span(shutter, t0, t1, H)
    scene = host.animated(W, H, variant, float(first), float(last))
    return scene, dev.DeviceScene(scene)


def kernel_of_last_launch(dev):
    L = dev.lib()
    return L.wpt_kernel_name().decode(), L.wpt_kernel_form().decode()


def test_zero_row_time_is_the_plain_render(dev):
    none = host.shutter(0.0)
    p = cases.params(0.0, 1.0)
    ds = dev.DeviceScene(host.animated(W, H, 0, 0.0, 1.0))
    plain, _ = ds.render(S, params=p)
    plain_kernel = kernel_of_last_launch(dev)
    got, _ = ds.render_shutter(S, none, params=p)
    assert kernel_of_last_launch(dev) == plain_kernel
    assert differing(got, plain) == 0 and np.isfinite(got).all() and got.sum() > 0
    # a scene at rest stays in its kernel with the scene in LDS
    ds = dev.DeviceScene(host.cornell(W, H, 1, 2))
    plain, _ = ds.render(S)
    plain_kernel = kernel_of_last_launch(dev)
    got, _ = ds.render_shutter(S, none)
    assert kernel_of_last_launch(dev) == plain_kernel
    assert "rotated corners" in plain_kernel[1]  # (a form that only the kernels with the scene in LDS have)
    assert differing(got, plain) == 0 and got.sum() > 0


@pytest.mark.parametrize("from_top", [True, False], ids=["from_top", "from_bottom"])
@pytest.mark.parametrize("variant", [0, 1, 8])
def test_rows_equal_plain_renders_and_the_restatement(dev, oracle, variant, from_top):
    """t0 < t1: every ray draws its time in its row's interval (variant 1, thin lens: one more draw in front of it; variant 8:
    marbles and a moving sphere light)"""
    t0, t1 = F32(0.0), F32(0.25)
    sh = host.shutter(ROW_TIME, from_top)
    scene, ds = rolling_scene(dev, variant, sh, t0, t1)
    got, _ = ds.render_shutter(S, sh, params=cases.params(t0, t1))
    assert np.isfinite(got).all() and got.sum() > 0
    rows = cases.intervals(sh, t0, t1)
    assert len({(float(a), float(b)) for a, b in rows}) == H
    for r, (a, b) in enumerate(rows):
        p = cases.params(a, b)
        plain, _ = ds.render(S, params=p)
        assert differing(got[r], plain[r]) == 0, ("device", variant, from_top, r, differing(got[r], plain[r]))
        ref, _ = oracle.render(scene, S, p, block=(r * W, W))
        assert differing(got[r], ref[r]) == 0, ("restatement", variant, from_top, r, differing(got[r], ref[r]))
    # it rolls: the frame is not the global-shutter frame of any one row's interval
    first_read = H - 1 if from_top else 0
    plain, _ = ds.render(S, params=cases.params(t0, t1))
    assert differing(got[first_read], plain[first_read]) == 0
    assert sum(differing(got[r], plain[r]) != 0 for r in range(H)) >= H // 2


def test_instant_rows_with_a_camera_at_rest(dev, oracle):
    """t0 == t1: no time is drawn, a row's rays all have the row's time; variant 2: only the scene moves"""
    t = F32(0.125)
    sh = host.shutter(F32(0.8) / F32(23), True)
    scene, ds = rolling_scene(dev, 2, sh, t, t)
    got, _ = ds.render_shutter(S, sh, params=cases.params(t, t))
    rows = cases.intervals(sh, t, t)
    assert all(a == b for a, b in rows) and len({float(a) for a, _ in rows}) == H
    for r, (a, _) in enumerate(rows):
        plain, _ = ds.render(S, params=cases.params(a, a))
        assert differing(got[r], plain[r]) == 0, (r, differing(got[r], plain[r]))
        ref, _ = oracle.render(scene, S, cases.params(a, a), block=(r * W, W))
        assert differing(got[r], ref[r]) == 0, ("restatement", r)
    still, _ = ds.render(S, params=cases.params(t, t))  # the global shutter at t: the row read first, and few others
    assert differing(got[H - 1], still[H - 1]) == 0 and sum(differing(got[r], still[r]) != 0 for r in range(H)) >= H // 2


def test_instant_rows_with_a_moving_camera(dev):
    """t0 == t1, variant 4 (instances at rest: only the pose matters): row r is taken where the camera's animation has it at
    a_r.  The plain render takes a camera's record, which holds Camera::at(t0) of the host; so row r is held to view 0 of a
    batch on the same uploaded scene, from the record of host.animated(..., a_r, a_r).  That rests on host Camera::at and
    device animationAt giving the same bits, which the anim_* pins assert; a failure here names the row and the differing
    words, and says which of the two to look at."""
    t = F32(0.0625)
    sh = host.shutter(F32(0.9) / F32(23), True)
    scene, ds = rolling_scene(dev, 4, sh, t, t)
    got, _ = ds.render_shutter(S, sh, params=cases.params(t, t))
    assert np.isfinite(got).all() and got.sum() > 0
    poses = set()
    for r, (a, _) in enumerate(cases.intervals(sh, t, t)):
        at_row = host.animated(W, H, 4, float(a), float(a))
        record = _abi.Camera.from_buffer_copy(at_row.camera.contents)
        assert record.animation == scene.camera.contents.animation >= 0
        poses.add(tuple(record.translation))
        view = ds.render_views(S, [record], params=cases.params(a, a))[0].cpu().numpy()
        bad = np.argwhere(cases.bits(got[r]) != cases.bits(view[r]))
        assert len(bad) == 0, "row %d (a = %r): %d words differ from the view of host Camera::at(a), first at %s: %r against %r; " \
            "device animationAt(a) or host Camera::at(a) is off" % (r, a, len(bad), bad[0], got[r][tuple(bad[0])], view[r][tuple(bad[0])])
    assert len(poses) == H  # the camera did move from row to row


@pytest.fixture(scope="module")
def rolling(dev):
    """the full rolling frame of variant 0 that blocks, bands and the counting launch are held to; read-only"""
    t0, t1 = F32(0.0), F32(0.25)
    sh = host.shutter(ROW_TIME, True)
    scene, ds = rolling_scene(dev, 0, sh, t0, t1)
    p = cases.params(t0, t1)
    frame, _ = ds.render_shutter(S, sh, params=p)
    frame.setflags(write=False)
    return scene, ds, sh, p, frame, (t0, t1)


def test_blocks_and_bands_keep_the_frames_rows(dev, rolling):
    import torch
    _, ds, sh, p, full, _ = rolling
    # a block that starts and ends mid-row
    start, size = 5 * W + 7, 3 * W + 11
    inside = np.zeros(W * H, dtype=bool)
    inside[start:start + size] = True
    block, _ = ds.render_shutter(S, sh, block=(start, size), params=p)
    assert differing(block.reshape(-1, 3)[inside], full.reshape(-1, 3)[inside]) == 0
    assert not block.reshape(-1, 3)[~inside].any()
    host_block = ds.render_shutter_host(S, sh, block=(start, size), params=p)
    assert host_block.shape == (size, 3) and differing(host_block, full.reshape(-1, 3)[inside]) == 0
    # bands of 8 rows, the second of every two: rows 8 .. 15 of this frame
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ds.render_shutter_bands_into(frame, S, sh, 8, 1, 2, params=p)
    torch.cuda.synchronize()
    ds.check()
    bands = frame.cpu().numpy()
    assert differing(bands[8:16], full[8:16]) == 0 and not bands[:8].any() and not bands[16:].any()
    host_bands = ds.render_shutter_host(S, sh, bands=(8, 1, 2), params=p)
    assert differing(host_bands, bands) == 0
    # ... and rows that are no multiple of 8, so that the launch is not tiled: bands 0 and 2 of 5 rows
    frame.zero_()
    ds.render_shutter_bands_into(frame, S, sh, 5, 0, 2, params=p)
    torch.cuda.synchronize()
    ds.check()
    bands = frame.cpu().numpy()
    mine = np.zeros(H, dtype=bool)
    for band in (0, 2, 4):
        mine[band * 5:band * 5 + 5] = True
    assert differing(bands[mine], full[mine]) == 0 and not bands[~mine].any()


def test_counting_launch(dev, rolling):
    """with_counters: the same frame from the counting build, and counters that are the sum over the rows of what the plain
    counting render of row r alone, with row r's interval, counts"""
    _, ds, sh, p, full, (t0, t1) = rolling
    got, counters = ds.render_shutter(S, sh, params=p, with_counters=True)
    assert differing(got, full) == 0
    total = dict.fromkeys(counters, 0)
    for r, (a, b) in enumerate(cases.intervals(sh, t0, t1)):
        _, row = ds.render(S, block=(r * W, W), params=cases.params(a, b), with_counters=True)
        for name in total:
            total[name] += row[name]
    assert counters == total and counters["samples"] == W * H * S * S


def test_refusals_come_back_from_the_render_calls(dev, rolling):
    _, ds, _, p, _, _ = rolling
    for name, sh, t0, t1, _, words in cases.bad_shutters():
        with pytest.raises(RuntimeError, match=words):
            ds.render_shutter(S, sh, params=cases.params(t0, t1))
        with pytest.raises(RuntimeError, match=words):
            ds.render_shutter_host(S, sh, bands=(8, 0, 1), params=cases.params(t0, t1))
    L = dev.lib()
    assert L.wpt_render_shutter_block_device(ds._handle, ds.host.camera, C.byref(p), None, W, H, S, 0, W * H, None, None, None) == 1
    assert "shutter is NULL" in L.wpt_last_error().decode()
    # sessions, the other sensors and batches of views have no shutter parameter
    for method in ("progressive", "render_stages", "render_transient_into", "render_light_groups_into", "render_tof_into", "render_adaptive_into",
                   "render_views_into", "render_view_streams_into", "render_split_into", "ground_truth_device"):
        assert "shutter" not in inspect.signature(getattr(dev.DeviceScene, method)).parameters, method


def test_example_runs(tmp_path):
    """examples/rolling_shutter.cpp at 48 x 32: exits 0 only if the row read first is the global-shutter render's bit for bit
    and other rows differ; two pictures"""
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "rolling_shutter")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rolling_shutter.cpp"),
                    "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, "48", "32", "3", str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    assert b"row read first equals the global shutter's" in r.stderr
    for name in ("global-shutter.png", "rolling-shutter.png"):
        assert os.path.getsize(str(tmp_path / name)) > 500
