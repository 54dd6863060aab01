"""Progressive sessions on the GPU (wurblpt_hip.h, wpt_progress_*): a frame rendered in stages of rows of strata is bit for bit
the one-shot frame and the oracle's, however the rows are cut, with a save and a restore in between, on a ragged block, with
the pixel pool and on two streams; previews are what the documented formula gives from the saved sums; and what sessions do
not cover is refused without harm to the next render."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
N = 5                                                       # samples_sqrt of the small scenes
PLANS = [[5], [1, 1, 1, 1, 1], [2, 3], [1, 100]]
HEADER = 224                                                # include/wurblpt_hip.h: the saved state's header, then 32 bytes per pixel


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from wurblpt_amd import device
    assert device.device_count() >= 1
    return device


def make_scene(name):
    p = None
    if name == "cornell":               # scene in LDS, rotated corners
        sc = host.cornell(48, 40, 1, 2)
    elif name == "triangles":           # scene in HBM, basic features, thin lens
        sc = host.random_triangles(1500, 5, with_texcoords=True, width=64, height=48, aperture=0.05)
    elif name == "sponza":              # all features
        sc = host.sponza_like(64, 48, seed=3, detail=0.03, tex_size=16, env_width=32, importance_n=8)
    elif name == "measured":            # measured BRDFs
        sc = host.measured_like(48, 40, host.rgl_fixture("iso"), host.rgl_fixture("aniso"), seed=5, detail=0.03, tex_size=16, env_width=32,
                                importance_n=8)
    else:                               # a moving scene with an exposure interval
        sc = host.animated(64, 48, 8, 0.0, 1.0)
        p = host.default_params()
        p.t0, p.t1 = 0.0, 1.0
    return sc, p


class Case:
    """a scene on the device with its two references, each computed once and left alone"""

    def __init__(self, dev, oracle, name):
        self.sc, self.params = make_scene(name)
        if self.sc.d.envmap.N > 0:
            tables = oracle.envmap_tables(self.sc)
            self.ds = dev.DeviceScene(self.sc)          # the device builds its own tables at upload
            self.sc.set_envmap_tables(*tables)
        else:
            self.ds = dev.DeviceScene(self.sc)
        self.w, self.h = self.sc.width, self.sc.height
        self.ref, _ = oracle.render(self.sc, N, self.params)
        dev.lib().wpt_set_wavefront(2, 0, 0, 0)
        try:
            self.oneshot, _ = self.ds.render(N, params=self.params)
            self.kernel = dev.lib().wpt_kernel_name()
        finally:
            dev.lib().wpt_set_wavefront(0, 0, 0, 0)
        assert bits_equal(self.oneshot, self.ref)


@pytest.fixture(scope="module")
def case(dev, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(dev, oracle, name)
        return made[name]
    return get


def saved_sums(state, size):
    """(sums float32 [size, 3], next stratum uint32 [size]) of a saved state, through the documented layout"""
    records = np.frombuffer(state, dtype=np.uint32, offset=HEADER).reshape(size, 8)
    return records[:, 4:7].view(np.float32), records[:, 7]


def run_plan(dev, c, plan, block=None, ds=None, session=None, sentinel=7.0):
    """renders the plan's stages; checks rows_done, the previews and that no stage but the last touches the frame.
    Returns (frame, last preview) as numpy arrays."""
    import torch
    ds = ds or c.ds
    start, size = block if block is not None else (0, c.w * c.h)
    s = session or ds.progressive(N, block=block, params=c.params)
    frame = torch.full((c.h, c.w, 3), sentinel, dtype=torch.float32, device="cuda")
    done = s.rows_done
    try:
        for rows in plan:
            last = done + rows >= N
            done = min(N, done + rows)
            assert s.advance(rows, frame if last else None) == done == s.rows_done
            assert dev.lib().wpt_last_render_passes() == 1
            assert dev.lib().wpt_kernel_name() == c.kernel
            out = torch.full((c.h, c.w, 3), sentinel, dtype=torch.float32, device="cuda")
            preview = s.preview(out).cpu().numpy().reshape(-1, 3)
            ds.check()
            assert np.all(preview[:start] == sentinel) and np.all(preview[start + size:] == sentinel)
            if not last:
                assert bool((frame == sentinel).all()), "a stage that does not finish the frame wrote to it"
                acc, stratum = saved_sums(s.save(), size)
                assert np.all(stratum == done << 16)
                want = np.float32(1) / np.float32(done * N) * acc
                assert bits_equal(preview[start:start + size], want), "preview after %d rows" % done
        assert s.finished
        got = frame.cpu().numpy()
        assert bits_equal(preview[start:start + size], got.reshape(-1, 3)[start:start + size]), "the finished session's preview is not its frame"
        return got, preview
    finally:
        s.close()


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("name", ["cornell", "triangles", "sponza", "measured", "animated"])
def test_staged_frame_is_the_one_shot_frame(dev, case, name, plan):
    c = case(name)
    fresh = c.ds.progressive(N, params=c.params)
    assert fresh.rows_done == 0 and fresh.rows_total == N and not fresh.finished
    assert not fresh.preview().cpu().numpy().any(), "a fresh session's preview is zeros"
    assert not np.frombuffer(fresh.save(), dtype=np.uint8, offset=HEADER).any()
    dev.lib().wpt_set_wavefront(1, 0, 0, 0)         # sessions never take the wavefront form
    try:
        got, _ = run_plan(dev, c, plan, session=fresh)
    finally:
        dev.lib().wpt_set_wavefront(0, 0, 0, 0)
    assert bits_equal(got, c.oneshot)
    assert bits_equal(got, c.ref)


@pytest.mark.parametrize("name", ["cornell", "triangles", "sponza", "measured", "animated"])
def test_save_close_and_resume_on_another_upload(dev, case, name):
    c = case(name)
    s = c.ds.progressive(N, params=c.params)
    s.advance(2)
    state = s.save()
    s.close()
    info = dev.progress_state_info(state)
    assert (info["width"], info["height"], info["samples_sqrt"], info["rows_done"], info["block_size"]) == (c.w, c.h, N, 2, c.w * c.h)
    assert info["tag"] == host.scene_tag(c.sc) and info["state_bytes"] == len(state)
    ds2 = dev.DeviceScene(c.sc)
    r = ds2.resume(state, params=c.params, samples_sqrt=N)
    assert r.rows_done == 2
    got, _ = run_plan(dev, c, [3], ds=ds2, session=r)
    assert bits_equal(got, c.oneshot)
    # a finished session's state still yields its frame
    s = c.ds.progressive(N, params=c.params)
    import torch
    frame = torch.zeros((c.h, c.w, 3), dtype=torch.float32, device="cuda")
    s.advance(N, frame)
    done = s.save()
    s.close()
    r = ds2.resume(done, params=c.params)
    assert r.finished and bits_equal(r.preview().cpu().numpy(), c.oneshot)
    r.close()
    ds2.close()


def test_restore_refuses_a_state_saved_with_something_else(dev, case):
    c = case("cornell")
    s = c.ds.progressive(N)
    s.advance(2)
    state = s.save()
    s.close()
    with pytest.raises(RuntimeError, match="samples_sqrt"):
        c.ds.resume(state, samples_sqrt=N + 1)
    other = host.default_params()
    other.max_path_components = 7
    with pytest.raises(RuntimeError, match="different params"):
        c.ds.resume(state, params=other)
    with pytest.raises(RuntimeError, match="different tag"):
        c.ds.resume(state, tag=host.scene_tag(c.sc) ^ 1)
    moved = host.cornell(48, 40, 1, 2)
    moved.camera.contents.translation[0] += 0.25
    ds2 = dev.DeviceScene(moved)
    with pytest.raises(RuntimeError, match="different camera"):
        ds2.resume(state)
    with pytest.raises(RuntimeError, match="carry"):
        c.ds.resume(state[:-1])
    # a damaged body: one pixel's next stratum is not the first of row 2
    record = HEADER + 32 * 1000
    damaged = state[:record + 28] + (3 << 16).to_bytes(4, "little") + state[record + 32:]
    with pytest.raises(RuntimeError, match=r"damaged.*pixel 1000.*status 1"):
        c.ds.resume(damaged)
    # the refusals left nothing behind: the state itself still resumes
    got, _ = run_plan(dev, c, [3], session=c.ds.resume(state))
    assert bits_equal(got, c.oneshot)


@pytest.mark.parametrize("name", ["cornell", "triangles"])
def test_ragged_block(dev, case, name):
    c = case(name)
    block = (37, c.w * c.h - 101)
    got, _ = run_plan(dev, c, [2, 3], block=block, sentinel=-3.0)
    flat = got.reshape(-1, 3)
    want, _ = c.ds.render(N, block=block, params=c.params)
    assert bits_equal(flat[37:37 + block[1]], want.reshape(-1, 3)[37:37 + block[1]])
    assert np.all(flat[:37] == -3.0) and np.all(flat[37 + block[1]:] == -3.0)


@pytest.mark.parametrize("name,sqrt,plan", [("cornell", 3, [1, 2]), ("triangles", 2, [1, 1])])
def test_with_the_pixel_pool(dev, oracle, name, sqrt, plan):
    """more pixels than the device holds lanes: every stage draws its pixels from the pool.  The one-shot launch of the Cornell
    frame goes through the twin that hands pixels out in slices, so this compares with a differently scheduled launch."""
    import torch
    w, h = 1024, 512
    sc = host.cornell(w, h, 1, 2) if name == "cornell" else host.random_triangles(1500, 5, with_texcoords=True, width=w, height=h, aperture=0.05)
    ds = dev.DeviceScene(sc)
    want, _ = ds.render(sqrt)
    s = ds.progressive(sqrt)
    frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    for rows in plan:
        s.advance(rows, frame)
        assert dev.lib().wpt_last_render_passes() == 1
    ds.check()
    got = frame.cpu().numpy()
    assert s.finished and bits_equal(s.preview().cpu().numpy(), got)
    s.close()
    assert bits_equal(got, want)
    rows_ref, _ = oracle.render(sc, sqrt, block=(100 * w, 2 * w))
    assert bits_equal(got[100:102], rows_ref[100:102])


def test_refusals_leave_the_next_render_alone(dev, case):
    import torch
    c = case("cornell")
    L = dev.lib()
    frame = torch.zeros((c.h, c.w, 3), dtype=torch.float32, device="cuda")

    def plain_render_is_right():
        got, _ = c.ds.render(N)
        assert bits_equal(got, c.ref)

    s = c.ds.progressive(N)
    with pytest.raises(RuntimeError, match=r"rows is 0.*status 1"):
        s.advance(0, frame)
    plain_render_is_right()
    s.advance(2)
    with pytest.raises(RuntimeError, match=r"frame_device.*status 1"):
        s.advance(3)                                        # the finishing stage without a frame
    assert s.rows_done == 2
    plain_render_is_right()
    s.advance(3, frame)
    with pytest.raises(RuntimeError, match=r"finished.*status 1"):
        s.advance(1, frame)
    plain_render_is_right()
    assert bits_equal(frame.cpu().numpy(), c.ref)
    s.close()
    for kwargs, word in [(dict(with_counters=True), "counting"), (dict(bands=True), "bands"), (dict(sensor=dev.SENSOR_TRANSIENT), "transient"),
                         (dict(sensor=dev.SENSOR_VIEWS), "views"), (dict(sensor=dev.SENSOR_ADAPTIVE), "adaptive"),
                         (dict(sensor=dev.SENSOR_TOF), "time-of-flight")]:
        with pytest.raises(RuntimeError, match=word + r".*status 4"):
            c.ds.progressive(N, **kwargs)
        plain_render_is_right()
    handle = C.c_void_p()
    p = host.default_params()
    assert L.wpt_progress_begin(c.ds._handle, c.sc.camera, C.byref(p), c.w, c.h, N, 10, c.w * c.h, 0, C.byref(handle)) == 1
    assert b"outside the frame" in L.wpt_last_error() and not handle.value
    plain_render_is_right()


def test_two_sessions_on_two_streams(dev, case):
    import torch
    c = case("triangles")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = [torch.zeros((c.h, c.w, 3), dtype=torch.float32, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    sessions = [c.ds.progressive(N, params=c.params) for _ in streams]
    plans = [[1, 1, 1, 1, 1], [2, 1, 2, 0, 0]]
    for stage in range(5):
        for s, st, fr, plan in zip(sessions, streams, frames, plans):
            if plan[stage]:
                s.advance(plan[stage], fr, st)
    previews = [s.preview(stream=st) for s, st in zip(sessions, streams)]
    torch.cuda.synchronize()
    c.ds.check()
    for s, fr, pv in zip(sessions, frames, previews):
        assert s.finished
        assert bits_equal(fr.cpu().numpy(), c.oneshot) and bits_equal(pv.cpu().numpy(), c.oneshot)
        s.close()


def test_render_stages_generator(dev, case):
    c = case("cornell")
    stages = [(rows, image.cpu().numpy()) for rows, image in c.ds.render_stages(N, rows_per_stage=2)]
    assert [rows for rows, _ in stages] == [2, 4, 5]
    assert bits_equal(stages[-1][1], c.oneshot)
    assert not bits_equal(stages[0][1], c.oneshot) and np.isfinite(stages[0][1]).all()
    # by time: the first stage renders one row; a stage as long as one likes then renders the rest, one as short as can be one row each
    assert [rows for rows, _ in c.ds.render_stages(N, seconds_per_stage=1e9)] == [1, 5]
    short = list(c.ds.render_stages(N, seconds_per_stage=1e-12))
    assert [rows for rows, _ in short] == [1, 2, 3, 4, 5] and bits_equal(short[-1][1].cpu().numpy(), c.oneshot)


def test_host_forms(dev, case):
    """wpt_progress_advance and wpt_progress_preview: host buffers in wpt_render_block's layout"""
    c = case("triangles")
    L = dev.lib()
    start, size = 37, c.w * c.h - 101
    handle = C.c_void_p()
    assert L.wpt_progress_begin(c.ds._handle, c.sc.camera, C.byref(c.params or host.default_params()), c.w, c.h, N, start, size, 5, C.byref(handle)) == 0
    block = np.full((size, 3), 9.0, np.float32)
    assert L.wpt_progress_advance(handle, 2, None) == 0 and L.wpt_progress_rows_done(handle) == 2
    assert L.wpt_progress_advance(handle, 3, None) == 1     # the finishing stage needs the buffer
    assert L.wpt_progress_advance(handle, 3, C.c_void_p(block.ctypes.data)) == 0
    want = c.oneshot.reshape(-1, 3)[start:start + size]
    assert bits_equal(block, want)
    preview = np.zeros((size, 3), np.float32)
    assert L.wpt_progress_preview(handle, C.c_void_p(preview.ctypes.data)) == 0
    assert bits_equal(preview, want)
    L.wpt_progress_end(handle)


def read_tgd(path):
    data = open(path, "rb").read()
    line, rest = data.split(b"\n", 1)
    tag, w, h, comps, kind = line.split()
    assert tag == b"WPTARRAY1" and kind == b"2"
    return np.frombuffer(rest, np.float32).reshape(int(h), int(w), int(comps))


def test_progressive_example_runs(tmp_path):
    """examples/progressive.cpp builds as the other examples do, and at 64x48: its staged frame and its frame resumed from the
    checkpoint file are the frame of plain mcpt()."""
    exe = str(tmp_path / "progressive")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "progressive.cpp"), "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, "64", "48", "5", "2", str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    assert "resumed at 2 of 5 rows" in out and "are bit for bit the frame of mcpt()" in out
    plain = read_tgd(str(tmp_path / "plain.tgd"))
    assert plain.shape == (48, 64, 3) and plain.any()
    assert bits_equal(read_tgd(str(tmp_path / "progressive.tgd")), plain)
    assert bits_equal(read_tgd(str(tmp_path / "progressive-resumed.tgd")), plain)
    for rows in (2, 4, 5):
        assert os.path.getsize(str(tmp_path / ("preview-%02d.png" % rows))) > 100
    from wurblpt_amd import device
    info = device.progress_state_info(open(str(tmp_path / "progressive.ckpt"), "rb").read())
    assert (info["width"], info["height"], info["samples_sqrt"], info["rows_done"]) == (64, 48, 5, 2)
