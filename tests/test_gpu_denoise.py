"""The denoiser on the GPU: wpt_postproc_denoise gives the bits of its host twin, colour and variance plane, for the frames of
tests/denoise_check.cpp and frames around one LDS tile, with every iteration count (so every step in each of its forms, with tiles
partly outside the frame), on a stream of its own, and leaves its inputs alone; a Cornell box rendered, guided and filtered
without leaving the device equals the host twin fed with the downloaded arrays; and the filtered 16-spp frame is closer to a
converged render than the noisy one, by the margin profiles/denoise_quality.txt measured."""
import numpy as np
import pytest

from tests import denoise_cases as cases
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

TILE = (32, 16)                                         # wpt_k_denoise.hip's TILE_W x TILE_H
AROUND_A_TILE = ((31, 15), (32, 16), (33, 17), (31, 17), (65, 15))
# relative L2 error of the filtered frame over that of the noisy one, Cornell 64 x 64 at 16 spp against 2304 spp with the default
# parameters: profiles/denoise_quality.txt measured MEASURED_RATIO; the bound lies halfway between it and 1
MEASURED_RATIO = 0.9649
QUALITY_BOUND = (MEASURED_RATIO + 1.0) / 2


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_steps_take_both_forms_or_one(dev):
    """the test below runs every step; this says which forms that covers"""
    forms = [dev.denoise_form(1 << i) for i in range(9)]
    print("forms of the steps 1 .. 256:", forms)
    assert set(forms) <= {"tile", "gather"} and "gather" in forms


@pytest.mark.parametrize("kind,size", [("mixed", s) for s in cases.SIZES + AROUND_A_TILE] + [("sky", (33, 9)), ("sky", (130, 70)),
                                                                                              ("unsampled", (5, 3)), ("unsampled", (130, 70))])
def test_device_equals_host_twin(dev, kind, size):
    import torch
    w, h = size
    c = cases.inputs(w, h, kind, seed=11)
    names = ("frame", "moments", "samples_sqrt", "positions", "normals", "materials")
    on_device = {k: torch.from_numpy(c[k].view(np.int16) if k == "samples_sqrt" else c[k]).cuda() for k in names}
    on_device["samples_sqrt"] = on_device["samples_sqrt"].view(torch.uint16)
    before = {k: t.clone() for k, t in on_device.items()}
    guide = (on_device["positions"], on_device["normals"], on_device["materials"])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for iterations in range(9):
        p = _abi.DenoiseParams(iterations=iterations)
        got, var = dev.denoise(on_device["frame"], on_device["moments"], on_device["samples_sqrt"], guide, p, variance_out=True, stream=stream)
        alone = dev.denoise(on_device["frame"], on_device["moments"], on_device["samples_sqrt"], guide, p, stream=stream)
        stream.synchronize()
        want, want_var = dev.denoise_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), p, variance_out=True)
        assert bits_equal(got.cpu().numpy(), want) and bits_equal(var.cpu().numpy(), want_var), (kind, size, iterations)
        assert bits_equal(alone.cpu().numpy(), want)
        assert np.isfinite(want).all() and np.isfinite(want_var).all()
    for k in names:
        assert torch.equal(on_device[k].view(torch.int16) if k == "samples_sqrt" else on_device[k],
                           before[k].view(torch.int16) if k == "samples_sqrt" else before[k]), k
    # one number stands for a constant map
    const = dev.denoise(on_device["frame"], on_device["moments"], 2, guide)
    torch.cuda.synchronize()
    assert bits_equal(const.cpu().numpy(), dev.denoise_host(c["frame"], c["moments"], 2, cases.guide(c)))


@pytest.fixture(scope="module")
def cornell(dev):
    """Cornell 64 x 64: the 16-spp frame with its moment film, the guide, the filtered frame (all on the device) and the
    2304-spp frame"""
    import torch
    sc = host.cornell(64, 64)
    ds = dev.DeviceScene(sc)
    m = np.full((64, 64), 4, np.uint16)
    frame, moments = ds.render_adaptive(m, with_moments=True)
    guide = ds.ground_truth_device()
    filtered, variance = dev.denoise(frame, moments, m, guide, variance_out=True)
    converged, _ = ds.render(48)
    torch.cuda.synchronize()
    ds.check()
    truth = dev.ground_truth(ds, bits=sum(1 << dev.GT_NAMES.index(n) for n in dev.GUIDE_NAMES))
    ds.close()
    return {"map": m, "frame": frame, "moments": moments, "guide": guide, "filtered": filtered, "variance": variance,
            "converged": np.asarray(converged).reshape(64, 64, 3), "truth": truth}


def test_rendered_guided_and_filtered_on_the_device(dev, cornell):
    guide = {k: v.cpu().numpy() for k, v in cornell["guide"].items()}
    assert sorted(guide) == sorted(dev.GUIDE_NAMES) and guide["materials"].dtype == np.int32
    for k in dev.GUIDE_NAMES:                             # the device tensors of the first-hit pass are the host form's arrays
        assert bits_equal(guide[k].reshape(64, 64, -1), cornell["truth"][k].reshape(64, 64, -1)), k
    want, want_var = dev.denoise_host(cornell["frame"].cpu().numpy(), cornell["moments"].cpu().numpy(), cornell["map"], guide, variance_out=True)
    assert bits_equal(cornell["filtered"].cpu().numpy(), want) and bits_equal(cornell["variance"].cpu().numpy(), want_var)
    assert not bits_equal(want, cornell["frame"].cpu().numpy()) and np.isfinite(want).all()


def test_the_filtered_frame_is_closer_to_the_converged_one(cornell):
    ref = cornell["converged"].astype(np.float64)
    error = lambda f: float(np.sqrt(((f.cpu().numpy().astype(np.float64) - ref) ** 2).sum() / (ref ** 2).sum()))
    noisy, filtered = error(cornell["frame"]), error(cornell["filtered"])
    print("relative L2 against 2304 spp: noisy %.5f, filtered %.5f, ratio %.4f" % (noisy, filtered, filtered / noisy))
    assert filtered < noisy
    assert filtered / noisy <= QUALITY_BOUND
