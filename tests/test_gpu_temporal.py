"""Temporal accumulation on the GPU: wpt_postproc_temporal_accumulate gives the bits of its host twin, every word of the history and
the length plane, over three-frame chains in every kind of motion with the device's own history fed back, for the frames of
tests/temporal_check.cpp and frames around one tile and one workgroup, and leaves its inputs and the previous history alone;
the filter on a history gives its host twin's bits and, on a first frame's history, the denoiser's; four rendered frames of a
Cornell box at rest accumulate to the mean of their sixteen sample streams and lie closer to a converged render than one frame;
two rendered frames of the animated room, guided and moved by the ground truth pass, equal the host twin fed with the downloaded
arrays, and history survives in some pixels and is reset in others."""
import numpy as np
import pytest

from tests import denoise_cases as cases
from tests import temporal_cases as tc
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def upload(a):
    import torch
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(t, before):
    import torch
    return torch.equal(t.view(torch.int16), before.view(torch.int16)) if t.dtype == torch.uint16 else torch.equal(t.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("kind", tc.MOTIONS)
@pytest.mark.parametrize("size", tc.GPU_SIZES)
def test_device_equals_host_twin(dev, size, kind):
    import torch
    w, h = size
    stream = torch.cuda.Stream()
    device_history = host_history = None
    for k, (f, g, motion) in enumerate(tc.chain(w, h, kind)):
        arrays = [upload(f[name]) for name in ("frame", "moments", "samples_sqrt")] + [upload(g[name]) for name in ("positions", "normals", "materials")]
        moved = None if motion is None else tuple(upload(a) for a in motion)
        held = [t.clone() for t in arrays + list(moved or ()) + ([device_history] if device_history is not None else [])]
        torch.cuda.synchronize()
        launch = stream if k == 1 else None                # the middle frame on a stream of its own
        got, length = dev.temporal_accumulate(arrays[0], arrays[1], arrays[2], tuple(arrays[3:]), moved, device_history, length_out=True, stream=launch)
        alone = dev.temporal_accumulate(arrays[0], arrays[1], arrays[2], tuple(arrays[3:]), moved, device_history, stream=launch)
        (launch or torch.cuda.current_stream()).synchronize()
        want, want_length = dev.temporal_accumulate_host(f["frame"], f["moments"], f["samples_sqrt"], cases.guide(g), motion, host_history, length_out=True)
        assert bits_equal(got.cpu().numpy(), want), (size, kind, k)
        assert bits_equal(length.cpu().numpy(), want_length) and bits_equal(alone.cpu().numpy(), want), (size, kind, k)
        assert np.isfinite(want[2]).all() and (want[2, ..., 3] >= 0).all()
        for t, before in zip(arrays + list(moved or ()) + ([device_history] if device_history is not None else []), held):
            assert same(t, before), "an input or the previous history was written"
        device_history, host_history = got, want
    N = host_history[1, ..., 3]
    if w * h > 500 and kind != "none":                     # history survives in some pixels and is lost in others
        assert (N > 1).any() and (N == 1).any()


@pytest.mark.parametrize("size", tc.GPU_SIZES)
def test_filtering_a_history(dev, size):
    """denoise_history is its host twin bit for bit, frame and variance, for 0, 1 and 5 iterations, on a history that motion made;
    on a first frame's history it is the denoiser itself; the history is not written"""
    import torch
    w, h = size
    history = None
    for f, g, motion in tc.chain(w, h, "random"):
        history = dev.temporal_accumulate_host(f["frame"], f["moments"], f["samples_sqrt"], cases.guide(g), motion, history)
    c = cases.inputs(w, h, "mixed", seed=11)
    on_device = [upload(c[k]) for k in ("frame", "moments", "samples_sqrt", "positions", "normals", "materials")]
    first = dev.temporal_accumulate(on_device[0], on_device[1], on_device[2], tuple(on_device[3:]))
    moved = upload(history)
    held = moved.clone(), first.clone()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for iterations in (0, 1, 5):
        p = _abi.DenoiseParams(iterations=iterations)
        got, var = dev.denoise_history(moved, p, variance_out=True, stream=stream)
        alone = dev.denoise_history(moved, p, stream=stream)
        stream.synchronize()
        want, want_var = dev.denoise_history_host(history, p, variance_out=True)
        assert bits_equal(got.cpu().numpy(), want) and bits_equal(var.cpu().numpy(), want_var) and bits_equal(alone.cpu().numpy(), want), (size, iterations)
        a, av = dev.denoise_history(first, p, variance_out=True)
        b, bv = dev.denoise(on_device[0], on_device[1], on_device[2], tuple(on_device[3:]), p, variance_out=True)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(av.view(torch.int32), bv.view(torch.int32)), (size, iterations)
    assert same(moved, held[0]) and same(first, held[1]), "the filter wrote the history"


@pytest.fixture(scope="module")
def cornell(dev):
    """Cornell 32 x 32 at rest: four frames of 4 streams x 2^2 samples from the streams 4f .. 4f + 3 with their stream moment films,
    accumulated on the device with the guide of the first-hit colour pass; the mean of the same sixteen streams; a 2304-spp frame"""
    import torch
    size = 32
    sc = host.cornell(size, size)
    ds = dev.DeviceScene(sc)
    guide = ds.first_hit_colours_device()
    frames, history, length = [], None, None
    for f in range(4):
        frame = torch.zeros((size, size, 3), dtype=torch.float32, device="cuda")
        moments = torch.zeros_like(frame)
        ds.render_split_into(frame, 2, 4, first=4 * f, moments=moments)
        history, length = dev.temporal_accumulate(frame, moments, 2, guide, None, history, length_out=True)
        frames.append(frame)
    accumulated, variance = dev.denoise_history(history, _abi.DenoiseParams(iterations=0), variance_out=True)
    torch.cuda.synchronize()
    ds.check()
    sixteen = ds.render_split(2, 16, first=0)
    converged, _ = ds.render(48)
    ds.close()
    return {"frames": [f.cpu().numpy() for f in frames], "history": history.cpu().numpy(), "length": length.cpu().numpy(),
            "accumulated": accumulated.cpu().numpy(), "variance": variance.cpu().numpy(), "sixteen": np.asarray(sixteen).reshape(size, size, 3),
            "converged": np.asarray(converged).reshape(size, size, 3)}


def test_rendered_at_rest(cornell):
    """N = 4 everywhere; the accumulated frame lies within 16 * 2^-24 * max|the four frames' values at that pixel and channel| of
    render_split(streams=16, first=0), the mean of the same sixteen streams; its relative L2 error against 2304 spp is below the
    single frame's (only the ordering is asserted; the statistics promise a factor near 1/2)"""
    assert (cornell["length"] == 4).all() and (cornell["history"][1, ..., 3] == 4).all()
    assert bits_equal(cornell["accumulated"], cornell["history"][2, ..., :3]) and bits_equal(cornell["variance"], cornell["history"][2, ..., 3])
    scale = np.abs(np.stack(cornell["frames"])).max(axis=0).astype(np.float64)
    off = np.abs(cornell["accumulated"].astype(np.float64) - cornell["sixteen"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print("accumulated against the mean of sixteen streams: %.3g of 2^-24 max" % np.nanmax(np.where(scale > 0, off / scale, 0) / EPS))
    assert (off <= 16 * EPS * scale).all()
    ref = cornell["converged"].astype(np.float64)
    error = lambda f: float(np.sqrt(((f.astype(np.float64) - ref) ** 2).sum() / (ref ** 2).sum()))
    single, accumulated = error(cornell["frames"][3]), error(cornell["accumulated"])
    print("relative L2 against 2304 spp: one frame %.5f, four accumulated %.5f, ratio %.4f" % (single, accumulated, accumulated / single))
    assert accumulated < single
    assert np.isfinite(cornell["variance"]).all() and (cornell["variance"] >= 0).all()


def test_rendered_moving(dev):
    """host.animated 40 x 32, static camera, moving instances, two frames 1 / 30 apart: guide and both offset arrays of the ground
    truth pass with times = (t, t - 1 / 30, t); the device's history equals the host form's on the downloaded arrays, bit for bit;
    history survives in some pixels (N = 2) and is reset in others (N = 1)"""
    import torch
    w, h, t, dt = 40, 32, 0.5, 1.0 / 30
    bits = sum(1 << dev.GT_NAMES.index(n) for n in dev.GUIDE_NAMES + dev.MOTION_NAMES)
    history = host_history = None
    for k, time in enumerate((t - dt, t)):
        sc = host.animated(w, h, 2, time, time)
        ds = dev.DeviceScene(sc)
        p = host.default_params()
        p.t0 = p.t1 = time
        truth = ds.ground_truth_device(bits=bits, params=p, times=(time, time - dt, time))
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        moments = torch.zeros_like(frame)
        ds.render_split_into(frame, 2, 4, first=4 * k, moments=moments, params=p)
        history, length = dev.temporal_accumulate(frame, moments, 2, truth, truth if k else None, history, length_out=True)
        torch.cuda.synchronize()
        ds.check()
        ds.close()
        arrays = {name: a.cpu().numpy() for name, a in truth.items()}
        host_history = dev.temporal_accumulate_host(frame.cpu().numpy(), moments.cpu().numpy(), 2, arrays, arrays if k else None, host_history)
        assert bits_equal(history.cpu().numpy(), host_history), k
        assert bits_equal(length.cpu().numpy(), host_history[1, ..., 3])
    N = host_history[1, ..., 3]
    moving = np.abs(arrays["pixel_space_offset_to_prev"]).max(axis=2) > 0
    print("N = 2 in %d pixels, N = 1 in %d of %d; %d pixels moved, by at most %.3f pixels" % ((N == 2).sum(), (N == 1).sum(), w * h, moving.sum(),
                                                                                           np.abs(arrays["pixel_space_offset_to_prev"]).max()))
    assert set(np.unique(N)) <= {1.0, 2.0}
    assert (N == 2).any() and (N == 1).any()
