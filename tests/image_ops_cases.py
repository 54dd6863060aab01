"""The fixtures of the image operations (tests/golden/image_ops/, written by tests/image_ops_cases.cpp over the reference's own
functions) for the CPU and the GPU tests: each case's input, the reference's output, and the call of the host or the device form
that must reproduce it."""
import json
import os

import numpy as np

from wurblpt_amd import device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_ops")
OPS = ("resample", "warp", "despeckle", "coords")
_LOADED = None


def _float(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def load():
    """(cases, data): the index's entries and the floats they point into; read once and left unchanged"""
    global _LOADED
    if _LOADED is None:
        cases = json.load(open(os.path.join(GOLDEN, "index.json")))
        data = np.fromfile(os.path.join(GOLDEN, "data.bin"), np.float32)
        data.setflags(write=False)
        _LOADED = (cases, data)
    return _LOADED


def names():
    return [c["name"] for c in load()[0]]


def case(name):
    return next(c for c in load()[0] if c["name"] == name)


def image_of(c):
    return load()[1][c["in"]:c["in"] + c["w"] * c["h"] * c["c"]].reshape(c["h"], c["w"], c["c"])


def expected_of(c):
    return load()[1][c["out"]:c["out"] + c["out_w"] * c["out_h"] * c["out_c"]].reshape(c["out_h"], c["out_w"], c["out_c"])


def camera_of(c):
    k = [_float(b) for b in c["k"]]
    return host.lens_camera([_float(b) for b in c["frustum"]], c["model"], *k)


def run(c, image, on_device, stream=None):
    """the case's operation on `image` (numpy for the host form, a CUDA tensor for the device form)"""
    extra = {"stream": stream} if on_device else {}
    pick = lambda name: getattr(device, name if on_device else name + "_host")
    if c["op"] == "resample":
        return pick("resample")(image, c["out_w"], c["out_h"], **extra)
    if c["op"] == "warp":
        return pick("lens_warp")(image, camera_of(c), bool(c["forward"]), **extra)
    if c["op"] == "despeckle":
        return pick("despeckle")(image, _float(c["min_factor"]), **extra)
    assert c["op"] == "coords"
    return pick("distance_to_coords")(image, camera_of(c), bool(c["pmd"]), **extra)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def digest(a):
    """sum of bit pattern k times (2 k + 1) modulo 2^64, as tests/image_ops_check.cpp prints it"""
    w = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    k = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return "%016x" % int((w * (np.uint64(2) * k + np.uint64(1))).sum(dtype=np.uint64))


def seeded(width, height, comps, seed, low=0.0, high=4.0):
    """a seeded random image [height, width, comps] of float32 in [low, high)"""
    rng = np.random.RandomState(seed)
    return (low + (high - low) * rng.rand(height, width, comps)).astype(np.float32)


def fireflies(width, height, seed):
    """a seeded quiet RGB frame with a firefly in about every twentieth pixel"""
    rng = np.random.RandomState(seed)
    frame = rng.rand(height, width, 3).astype(np.float32)
    hot = rng.rand(height, width) < 0.05
    frame[hot] *= np.float32(50.0)
    return frame


# the lenses of the seeded cases: (model, k1, k2, k3, p1, p2) on the fixtures' frustum
FRUSTUM = (-0.625, 0.75, -0.1875, 0.15625)
LENSES = {"none": (0, 0, 0, 0, 0, 0), "radial_and_planar": (1, 0.5, 0.125, 0.0, 0.03125, -0.015625),
          "radial_only": (2, 0.375, 0.0625, 0.015625, 0.0, 0.0), "opencv": (3, 0.25, 0.0625, 0.0078125, 0.015625, -0.0078125)}


def lens(name):
    return host.lens_camera(FRUSTUM, *LENSES[name])
