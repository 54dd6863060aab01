"""Inputs of the denoiser's tests (test_denoise_host.py, test_gpu_denoise.py): seeded frames with their moment films, sample-count
maps and guides, the frame sizes of tests/denoise_check.cpp, and that program's digest."""
import numpy as np

# width, height: one pixel, one column, fewer rows than taps, odd sizes around one tile, several tiles in both directions
SIZES = ((1, 1), (1, 7), (5, 3), (33, 9), (130, 70))
KINDS = ("mixed", "sky", "unsampled")
COUNTS = (0, 1, 2, 5)                                   # n_p: not rendered, no estimate, the smallest estimate, a usual one


def digest(values):
    """tests/denoise_check.cpp's: the sum over the 32-bit words w_k of w_k * (2 k + 1) modulo 2^64, 16 hexadecimal digits"""
    w = np.ascontiguousarray(values).reshape(-1).view(np.uint32).astype(np.uint64)
    k = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return "%016x" % int((w * (k * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))


def inputs(width, height, kind="mixed", seed=1):
    """dict frame, moments [h, w, 3] float32, samples_sqrt [h, w] uint16, positions, normals [h, w, 3] float32, materials [h, w]
    int32.  mixed: four materials in patches, each a plane seen at a slant with a rough surface and normals a few degrees around
    its own, a tenth of the pixels sky, n_p from COUNTS; sky: nothing hit anywhere; unsampled: n_p = 0 and a black frame."""
    rng = np.random.RandomState(seed * 1000003 + width * 131 + height)
    y, x = np.mgrid[0:height, 0:width]
    m = (((x // 3) * 7 + (y // 2) * 3) % 4).astype(np.int32)
    m[((x // 4 + y // 3) % 10) == 0] = -1
    if kind == "sky":
        m[:] = -1
    n_p = np.array(COUNTS, np.uint16)[rng.randint(0, 4, (height, width))]
    if kind == "unsampled":
        n_p[:] = 0
    frame = (rng.rand(height, width, 3) * 4).astype(np.float32)
    frame[rng.rand(height, width, 3) < 1 / 16] = 0
    frame[n_p == 0] = 0
    factor = np.where(rng.rand(height, width, 3) < 0.2, 0.5, 1.25 + rng.rand(height, width, 3)).astype(np.float32)
    moments = (frame * frame * factor).astype(np.float32)
    base = np.array([[0.1, 0.2, 1.0], [0.6, 0.0, 0.8], [-0.3, 0.3, 0.9], [0.0, -0.5, 0.85]])
    normals = base[np.maximum(m, 0)] + (rng.rand(height, width, 3) - 0.5) * 0.1
    normals /= np.linalg.norm(normals, axis=2, keepdims=True)
    depth = -2.0 - 0.5 * np.maximum(m, 0) - 0.01 * x - 0.02 * y + (rng.rand(height, width) - 0.5) * 0.004
    positions = np.stack([x / 32.0, y / 32.0, depth], axis=2)
    hit = (m >= 0)[..., None]
    return {"frame": frame, "moments": moments, "samples_sqrt": n_p, "positions": np.where(hit, positions, 0).astype(np.float32),
            "normals": np.where(hit, normals, 0).astype(np.float32), "materials": m}


def guide(case):
    return case["positions"], case["normals"], case["materials"]
