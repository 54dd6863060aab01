"""Sample streams on the GPU: the seed of stream k is pinned to the oracle through the lens-only camera for every kernel family of
the batch of views; stream 0 is the plain render; a split render is the host mean of its streams' frames; the device's mean and
merge are the host's; and the streams are independent (one statistical test)."""
import numpy as np
import pytest

from tests import streams_cases as cases
from tests.test_gpu_views import make_cameras
from wurblpt_amd import host

pytestmark = pytest.mark.gpu

PIXELS = cases.W * cases.H


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_pinned(dev, oracle, name, streams, oracle_height):
    """the lens-only camera rendered as `streams` in one launch against the oracle's blocks (k * 128, 128) of a 16 x oracle_height
    frame, and the counting launch's counters against the sum of the oracle's block counters"""
    _, _, variant, words, lens = cases.SCENES[name]
    sc, p = cases.make(name, oracle)
    cam = cases.lens_only_camera(sc, lens)
    dev.lib().wpt_set_launch_config(0, variant)
    try:
        ds = dev.DeviceScene(sc)
        frames = ds.render_view_streams(cases.S, [cam] * len(streams), streams=streams, params=p).cpu().numpy()
        kernel = dev.lib().wpt_kernel_name().decode()
        assert "views" in kernel and words in kernel, kernel
        assert dev.lib().wpt_last_render_passes() == 1
        counted, counters = ds.render_view_streams(cases.S, [cam] * len(streams), streams=streams, params=p, with_counters=True)
        assert "counting" in dev.lib().wpt_kernel_name().decode()
    finally:
        dev.lib().wpt_set_launch_config(0, 0)
    assert bits_equal(counted.cpu().numpy(), frames)
    total = None
    for v, k in enumerate(streams):
        ref, cnt = cases.with_camera(sc, cam, lambda: cases.oracle_block(oracle, sc, p, cases.W, oracle_height, k * PIXELS, PIXELS))
        got = frames[v].reshape(-1, 3)
        nbad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        assert nbad == 0, "stream %d: %d of %d values differ from the oracle's block" % (k, nbad, got.size)
        total = cnt if total is None else {key: total[key] + cnt[key] for key in total}
    assert counters == total, (counters, total)
    return frames


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_the_seed_of_a_stream_is_the_oracles(dev, oracle, name):
    frames = check_pinned(dev, oracle, name, [0, 1, 2], 24)
    assert np.isfinite(frames).all() and not bits_equal(frames[1], frames[0]) and not bits_equal(frames[2], frames[0])


@pytest.mark.parametrize("name", ["cornell", "cornell_lds"])
def test_unordered_and_large_streams(dev, oracle, name):
    """streams (5, 0, 70000): the index 70000 * 128 + p lies in a 16 x 560008 frame, of which the oracle renders the blocks only"""
    check_pinned(dev, oracle, name, [5, 0, 70000], 560008)


def test_stream_zero_is_the_plain_render(dev):
    sc = host.cornell(37, 23, 1, 2)
    cams = make_cameras(sc, ["scene", "pose", "pose"])
    ds = dev.DeviceScene(sc)
    plain = ds.render_views(2, cams).cpu().numpy()
    assert bits_equal(ds.render_view_streams(2, cams, streams=None).cpu().numpy(), plain)
    assert bits_equal(ds.render_view_streams(2, cams, streams=[0, 0, 0]).cpu().numpy(), plain)
    # stream 0 beside streams 1 and 2, in every position of the batch
    for zero_at in range(3):
        streams = [1, 2]
        streams.insert(zero_at, 0)
        mixed = ds.render_view_streams(2, cams, streams=streams).cpu().numpy()
        for v in range(3):
            assert bits_equal(mixed[v], plain[v]) == (v == zero_at), (zero_at, v)
            assert np.isfinite(mixed[v]).all() and mixed[v].any()


def test_a_split_render_is_the_mean_of_its_streams(dev):
    sc = host.cornell(37, 23, 1, 2)
    ds = dev.DeviceScene(sc)
    cam = cases._abi.Camera.from_buffer_copy(sc.camera.contents)
    frames = ds.render_view_streams(2, [cam] * 4, streams=[3, 4, 5, 6]).cpu().numpy()
    want_frame, want_moments = dev.mean_planes_host(frames, with_moment=True)
    frame, moments, counters = ds.render_split(2, streams=4, first=3, with_moments=True, with_counters=True)
    assert "views" in dev.lib().wpt_kernel_name().decode()
    assert bits_equal(frame, want_frame) and bits_equal(moments, want_moments)
    assert counters["samples"] == 4 * 37 * 23 * 4
    assert bits_equal(ds.render_split(2, streams=4, first=3), want_frame)           # without the moment film
    assert (moments >= frame * frame * np.float32(0.999)).all()                     # a mean of squares is no less than the mean's square
    # one stream from 0 is the plain render
    plain, _ = ds.render(2)
    assert bits_equal(ds.render_split(2, streams=1, first=0), plain)
    one, one_moments = ds.render_split(2, streams=1, first=0, with_moments=True)
    assert bits_equal(one, plain) and bits_equal(one_moments, plain * plain)


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_device_mean_and_merge_are_the_hosts(dev, K):
    import torch
    planes = cases.adversarial_planes(K)
    want_mean, want_moment = dev.mean_planes_host(planes, with_moment=True)
    d = torch.from_numpy(planes).cuda()
    mean, moment = dev.mean_planes(d, with_moment=True)
    assert cases.same_bits(mean.cpu().numpy(), want_mean) and cases.same_bits(moment.cpu().numpy(), want_moment)
    assert cases.same_bits(dev.mean_planes(d).cpu().numpy(), want_mean)
    other = torch.from_numpy(cases.adversarial_planes(K, seed=31)).cuda()
    for ca, cb in ((8, 8), (1, 3), (5, 0), (0xffffffff, 0xffffffff)):
        got = dev.merge_means(d[0], ca, other[K - 1], cb).cpu().numpy()
        assert cases.same_bits(got, dev.merge_means_host(planes[0], ca, other[K - 1].cpu().numpy(), cb)), (ca, cb)
    # in place: out may be a
    a = d[0].clone()
    want = dev.merge_means_host(planes[0], 2, other[0].cpu().numpy(), 6)
    assert dev.merge_means(a, 2, other[0], 6, out=a) is a and cases.same_bits(a.cpu().numpy(), want)


def test_render_split_writes_only_its_own_tensors(dev):
    import torch
    sc = host.cornell(37, 23, 1, 2)
    ds = dev.DeviceScene(sc)
    want, want_moments = ds.render_split(2, streams=4, with_moments=True)
    sentinel = float(np.frombuffer(np.uint32(0x7fc0beef).tobytes(), np.float32)[0])
    big = torch.full((3, 23, 37, 3), sentinel, dtype=torch.float32, device="cuda")
    big_moments = torch.full((3, 23, 37, 3), sentinel, dtype=torch.float32, device="cuda")
    ds.render_split_into(big[1], 2, 4, moments=big_moments[1], stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    ds.check()
    for t, w in ((big.cpu().numpy(), want), (big_moments.cpu().numpy(), want_moments)):
        for k in (0, 2):
            assert (t[k].view(np.uint32) == 0x7fc0beef).all(), "frame %d outside the render was written" % k
        assert bits_equal(t[1], w)


def test_the_streams_are_independent(dev):
    """The one statistical test.  Against R, the plain render at 32^2 spp: e_plain is the relative L2 error of the plain render
    at 8^2 spp, e_split that of 16 streams of 2^2 spp, the same 64 samples per pixel.  Independent streams give e_split near
    e_plain (a little above: the strata are coarser); sixteen identical or strongly correlated streams would give the error of
    4 samples, four times as much (error goes as 1 / sqrt(spp)).  Asserted is e_split <= 2 e_plain, the geometric mean of the
    two cases, and that no two of the sixteen stream frames are equal.  Measured: profiles/streams_quality.txt."""
    sc = host.cornell(24, 24, 1, 2)
    ds = dev.DeviceScene(sc)
    R = ds.render(32)[0].astype(np.float64)
    plain = ds.render(8)[0].astype(np.float64)
    split = ds.render_split(2, streams=16).astype(np.float64)
    norm = np.sqrt((R * R).sum())
    e_plain = np.sqrt(((plain - R) ** 2).sum()) / norm
    e_split = np.sqrt(((split - R) ** 2).sum()) / norm
    print("streams quality: e_plain %.5f e_split %.5f ratio %.3f" % (e_plain, e_split, e_split / e_plain))
    cam = cases._abi.Camera.from_buffer_copy(sc.camera.contents)
    frames = ds.render_view_streams(2, [cam] * 16, streams=list(range(16))).cpu().numpy()
    for i in range(16):
        for j in range(i + 1, 16):
            assert not bits_equal(frames[i], frames[j]), (i, j)
    assert bits_equal(dev.mean_planes_host(frames), split.astype(np.float32))
    assert e_plain > 0 and e_split <= 2.0 * e_plain, (e_plain, e_split)
