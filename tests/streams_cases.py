"""What the tests of sample streams share (tests/test_streams_host.py, tests/test_gpu_streams.py): the five scenes, the lens-only
camera that lets the oracle restate a stream, adversarial planes for the mean and the merge, and a comparison of float bits."""
import numpy as np

from wurblpt_amd import _abi, host

W, H, S = 16, 8, 2            # the frames the seed is pinned at: 128 pixels, 2^2 samples

SCENES = {
    # name: (scene, (t0, t1) or None, launch variant, words of the views kernel's name, the camera has its lens)
    # A thin lens takes the all-features kernels, so the two basic kernels get the same camera without it: an empty frustum
    # behind a pinhole, one primary ray for every sample of every pixel, and again a value that depends on the generator alone.
    "cornell_lds": (lambda w=W, h=H: host.cornell(w, h, 1, 2), None, 0, "scene in LDS", False),
    "basic_hbm": (lambda w=W, h=H: host.cornell(w, h, 1, 2), None, 0x01, "views, basic", False),
    "cornell": (lambda w=W, h=H: host.cornell(w, h, 1, 2), None, 0, "all features", True),
    "sponza_like": (lambda w=W, h=H: host.sponza_like(w, h, detail=0.05, tex_size=32, env_width=64, importance_n=16), None, 0, "all features", True),
    "spheres": (lambda w=W, h=H: host.spheres(w, h, 1), None, 0, "all features", True),
    "animated": (lambda w=W, h=H: host.animated(w, h, 8, 0.0, 1.0), (0.0, 1.0), 0, "moving scenes", True),
    "rgl_scene": (lambda w=W, h=H: host.rgl_scene(w, h, 1), None, 0, "measured BRDFs", True),
}
# the scenes and cameras of the premise (basic_hbm is cornell_lds again, rendered by another kernel)
PREMISE = ["cornell_lds", "cornell", "sponza_like", "spheres", "animated", "rgl_scene"]


def make(name, oracle):
    """(scene, params) of SCENES[name], ready for the oracle"""
    build, times = SCENES[name][:2]
    sc = build()
    if sc.d.envmap.N > 0 and not sc.d.envmap.M:
        sc.set_envmap_tables(*oracle.envmap_tables(sc))     # the oracle takes the importance tables from its caller
    p = host.default_params()
    if times is not None:
        p.t0, p.t1 = times
    return sc, p


def lens_only_camera(sc, lens=True):
    """A copy of the scene's camera with an empty frustum (l = r = b = t = 0) and a thin lens: every pixel shoots the same family
    of rays, so a pixel's value depends on its generator alone.  The oracle then restates stream k: pixel p of stream k of a
    w x h frame is pixel p + k * w * h of the oracle's render of any frame that holds that index.  lens=False: without the lens.
    (SCENES has why)"""
    cam = _abi.Camera.from_buffer_copy(sc.camera.contents)
    d = float(np.linalg.norm(np.array(cam.translation, np.float64)))
    cam.l = cam.r = cam.b = cam.t = 0.0
    cam.lens_radius = 0.05 * d if lens else 0.0
    cam.focus_dist = 0.5 * d if lens else cam.focus_dist
    return cam


def with_camera(sc, cam, fn):
    """fn() while the scene's camera is `cam` (the oracle and the plain render read it from the host scene)"""
    saved = _abi.Camera.from_buffer_copy(sc.camera.contents)
    sc.camera[0] = cam
    try:
        return fn()
    finally:
        sc.camera[0] = saved


def oracle_block(oracle, sc, params, width, height, first, count, samples_sqrt=S):
    """pixels [first, first + count) of the oracle's render of a width x height frame: (float32 [count, 3], counters)"""
    frame, counters = oracle.render(sc, samples_sqrt, params=params, block=(first, count), width=width, height=height)
    return frame.reshape(-1, 3)[first:first + count].copy(), counters


def adversarial_planes(K, seed=7):
    """float32 planes [K, 9, 7, 3]: values of both signs over many magnitudes, and +-inf, NaN, denormals and -0.0 among them"""
    rng = np.random.RandomState(seed + K)
    planes = (rng.standard_normal((K, 9, 7, 3)) * np.exp(rng.uniform(-12.0, 12.0, (K, 9, 7, 3)))).astype(np.float32)
    flat = planes.reshape(K, -1)
    specials = np.array([np.inf, -np.inf, np.nan, 1e-42, -3e-45, -0.0, 0.0, 3e38, -3e38], np.float32)
    for k in range(K):
        at = rng.choice(flat.shape[1], size=2 * len(specials), replace=False)
        flat[k, at] = np.tile(specials, 2)
    flat[:, 0] = -0.0                                       # a value that is -0.0 in every plane: the sum must not start from +0
    flat[:, 1] = np.float32(1e-42)                          # denormal in every plane
    return planes


def same_bits(a, b):
    """bit for bit, except that a NaN matches any NaN: IEEE 754 leaves the sign and payload of an operation's NaN to the
    implementation (x86 makes inf - inf a negative NaN, the GPU a positive one)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def mean_reference(planes, with_moment=False):
    """numpy's float32 evaluation of wpt_streams.h's mean (and moment) in the stated order, one rounding per operation"""
    K = planes.shape[0]
    with np.errstate(all="ignore"):
        total = planes[0].copy()
        squares = (planes[0] * planes[0]).astype(np.float32)
        for k in range(1, K):
            total = (total + planes[k]).astype(np.float32)
            squares = (squares + (planes[k] * planes[k]).astype(np.float32)).astype(np.float32)
        inv = np.float32(1.0) / np.float32(K)
        mean, moment = (total * inv).astype(np.float32), (squares * inv).astype(np.float32)
    return (mean, moment) if with_moment else mean
