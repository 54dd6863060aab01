"""Inputs of the tests of temporal accumulation (test_temporal_host.py, test_gpu_temporal.py), built on tests/denoise_cases.py:
sequences of seeded frames over one guide, whole-pixel, fractional and random motion with offsets that say so, and a float64
restatement of the rule (include/wurblpt_hip.h, "temporal accumulation") written from its description."""
import numpy as np

from tests import denoise_cases as cases

SIZES = cases.SIZES
GPU_SIZES = SIZES + ((63, 15), (64, 16), (65, 17))        # partial and whole tiles of the filter, partial and whole workgroups
MOTIONS = ("none", "zero", "whole", "fractional", "random")
MARGIN = 1e-4                                             # how far every validity decision of the built inputs stays from its threshold
KY = np.array([0.212671, 0.715160, 0.072169])


def sequence(width, height, count, seed=1, sampled=True):
    """(guide case, [frame dicts]): one guide of denoise_cases.inputs and `count` seeded frames over it, each with its moment film
    and its own sample-count map; sampled: n_p from {1, 2, 5}, else from denoise_cases.COUNTS (0 among them)"""
    g = cases.inputs(width, height, "mixed", seed)
    frames = []
    for k in range(count):
        rng = np.random.RandomState(seed * 7919 + k * 104729 + width * 131 + height)
        n_p = np.array((1, 2, 5) if sampled else cases.COUNTS, np.uint16)[rng.randint(0, 3 if sampled else 4, (height, width))]
        frame = (0.125 + rng.rand(height, width, 3) * 4).astype(np.float32)
        frame[n_p == 0] = 0
        moments = (frame * frame * (1.25 + rng.rand(height, width, 3))).astype(np.float32)
        frames.append({"frame": frame, "moments": moments, "samples_sqrt": n_p})
    return g, frames


def shifted(a, ox, oy):
    """a[y + oy, x + ox] where that lies in the frame (elsewhere a's own value), and the mask of where it does"""
    h, w = a.shape[:2]
    out = a.copy()
    valid = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        valid[y0:y1, x0:x1] = True
    return out, valid


def shifted_guide(g, ox, oy):
    """the guide whose pixel (x, y) shows what g shows at (x + ox, y + oy): the current guide of a frame whose previous guide is
    g, with the pixel offset (ox, oy) and the camera offset 0 everywhere.  Returns (guide, the mask of sources in the frame)."""
    out = {}
    for name in ("positions", "normals", "materials"):
        out[name], valid = shifted(g[name], ox, oy)
    return out, valid


def plane_offsets(g, offsets):
    """camera-space offsets that go with pixel offsets on the slanted planes of denoise_cases.inputs: a point seen (dx, dy) pixels
    away lay at P + (dx / 32, dy / 32, -0.01 dx - 0.02 dy)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.nan_to_num(offsets.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0).clip(-8, 8)
    return np.stack([d[..., 0] / 32, d[..., 1] / 32, -0.01 * d[..., 0] - 0.02 * d[..., 1]], axis=2).astype(np.float32)


def motion(g, kind, seed=3):
    """(pixel offsets [h, w, 2], camera offsets [h, w, 3]) float32 for a frame whose guide and whose previous guide are both g
    (None, None for "none").  zero: offsets 0; fractional: (0.37, -1.61) everywhere; random: per pixel from +-3, one in sixteen
    NaN, infinite or far outside the frame.  ("whole" is shifted_guide's.)"""
    h, w = g["materials"].shape
    if kind == "none":
        return None, None
    if kind == "zero":
        return np.zeros((h, w, 2), np.float32), np.zeros((h, w, 3), np.float32)
    if kind == "fractional":
        off = np.broadcast_to(np.array([0.37, -1.61], np.float32), (h, w, 2)).copy()
    else:
        assert kind == "random"
        rng = np.random.RandomState(seed * 31 + w * 131 + h)
        off = ((rng.rand(h, w, 2) - 0.5) * 6).astype(np.float32)
        odd = rng.randint(0, 16, (h, w)) == 0
        what = rng.randint(0, 4, (h, w))
        off[odd & (what == 0)] = np.nan
        off[odd & (what == 1), 0] = np.inf
        off[odd & (what == 2), 1] = -np.inf
        off[odd & (what == 3)] = (1e6, -3e5)
    return off, plane_offsets(g, off)


class Restated:
    """The rule in float64 for one frame: fx, fy, the floors and the tap weights in float32 as the rule defines them, everything
    else in float64.  `history`, `records`: [3, h, w, 4] float32 (the previous history; prepare()'s records of the current
    frame as a first-frame history holds them), `n_p` the current sample-count map, offsets as the call takes them.
    After construction: B_w, C [h, w, 4] float64 are the new records' words, `scale_c` [h, w, 4] and `scale_n` [h, w] the largest
    magnitude among the words that enter each output word, and `margin` the smallest relative distance of a validity decision
    from its threshold (pixels in `ignore` left out)."""

    def __init__(self, history, records, n_p, pixel, camera, max_history=32.0, normal_cos_min=0.9, tolerance=0.02):
        h, w = n_p.shape
        A, B, C = (records[k].astype(np.float64) for k in range(3))
        m = records[0][..., 3].view(np.int32)
        hA, hB, hC = (history[k].astype(np.float64) for k in range(3))
        hm = history[0][..., 3].view(np.int32)
        y, x = np.mgrid[0:h, 0:w]
        margins = np.full((h, w), np.inf)
        if pixel is None:
            source = np.ones((h, w), bool)
            ix, iy = x, y
            wx = [np.ones((h, w), np.float32), np.zeros((h, w), np.float32)]
            wy = [np.ones((h, w), np.float32), np.zeros((h, w), np.float32)]
            E = A[..., :3]
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                fx = x.astype(np.float32) + pixel[..., 0]
                fy = y.astype(np.float32) + pixel[..., 1]
                inside = (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
                source = inside & (m >= 0)
                for f, hi in ((fx, w), (fy, h)):   # the decision fx > -1 && fx < width: its distance from either threshold
                    near = np.minimum(np.abs(f.astype(np.float64) + 1), np.abs(f.astype(np.float64) - hi) / hi)
                    margins = np.minimum(margins, np.where(np.isfinite(f) & (m >= 0), near, np.inf))
            fx, fy = np.where(source, fx, 0).astype(np.float32), np.where(source, fy, 0).astype(np.float32)
            flx, fly = np.floor(fx), np.floor(fy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            wx1, wy1 = fx - flx, fy - fly
            wx = [np.float32(1) - wx1, wx1]
            wy = [np.float32(1) - wy1, wy1]
            assert all(a.dtype == np.float32 for a in wx + wy)
            E = A[..., :3] + camera.astype(np.float64)
        sw = np.zeros((h, w))
        sc = np.zeros((h, w, 4))
        sn = np.zeros((h, w))
        scale_c = np.abs(C)
        scale_n = np.ones((h, w))
        tol2EE = tolerance * tolerance * (E * E).sum(axis=2)
        for j in (0, 1):
            for i in (0, 1):
                wt = (wy[j] * wx[i]).astype(np.float32)
                qx, qy = ix + i, iy + j
                ok = source & (wt != 0) & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ok &= hm[cy, cx] == m
                cos = (B[..., :3] * hB[cy, cx, :3]).sum(axis=2)
                D = hA[cy, cx, :3] - E
                dd = (D * D).sum(axis=2)
                surface = ok & (m >= 0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    near = np.minimum(np.abs(cos - normal_cos_min) / max(abs(normal_cos_min), 1e-30), np.abs(dd - tol2EE) / tol2EE)
                margins = np.minimum(margins, np.where(surface, near, np.inf))
                ok &= (m < 0) | ((cos >= normal_cos_min) & (dd <= tol2EE))
                wt64 = np.where(ok, wt.astype(np.float64), 0)
                sw += wt64
                sc += wt64[..., None] * np.where(ok[..., None], hC[cy, cx], 0)
                sn += wt64 * np.where(ok, hB[cy, cx, 3], 0)
                scale_c = np.maximum(scale_c, np.where(ok[..., None], np.abs(hC[cy, cx]), 0))
                scale_n = np.maximum(scale_n, np.where(ok, hB[cy, cx, 3] + 1, 0))
        valid = sw > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            H = np.where(valid[..., None], sc / sw[..., None], 0)
            NH = np.where(valid, sn / sw, 0)
        N = np.minimum(NH + 1, max_history)
        a = 1 / N
        b = 1 - a
        mixed = np.concatenate([b[..., None] * H[..., :3] + a[..., None] * C[..., :3], (b * b * H[..., 3] + a * a * C[..., 3])[..., None]], axis=2)
        sampled = n_p > 0
        self.valid = valid
        self.C = np.where(valid[..., None], np.where(sampled[..., None], mixed, H), C)
        self.B_w = np.where(valid, np.where(sampled, N, NH), np.where(sampled, 1.0, 0.0))
        self.scale_c, self.scale_n = scale_c, scale_n
        self.margins = margins

    def margin(self, ignore=None):
        m = self.margins if ignore is None else np.where(ignore, np.inf, self.margins)
        return float(m.min())


def settle(history, records, n_p, pixel, camera, **params):
    """offsets with every pixel whose validity decisions lie within MARGIN of a threshold made NaN (a reset, which decides
    nothing), so that the built inputs keep the margin the tests assert"""
    pixel = pixel.copy()
    for _ in range(4):
        r = Restated(history, records, n_p, pixel, camera, **params)
        close = r.margins < 2 * MARGIN
        if not close.any():
            return pixel
        pixel[close] = np.nan
    raise AssertionError("the inputs do not settle")


def chain(width, height, kind, count=3):
    """`count` frames in one kind of MOTIONS: a list of (frame dict, guide dict, motion) with motion None or (pixel offsets, camera
    offsets); for "whole" every frame's guide is the one before shifted by (3, -2)"""
    g, frames = sequence(width, height, count, seed=5, sampled=False)
    out = []
    for k, f in enumerate(frames):
        if kind == "whole":
            if k > 0:
                g = shifted_guide(g, 3, -2)[0]
            m = (np.broadcast_to(np.array([3, -2], np.float32), (height, width, 2)).copy(), np.zeros((height, width, 3), np.float32))
        else:
            m = motion(g, kind, seed=3 + k)
        out.append((f, g, None if kind == "none" else m))
    return out
