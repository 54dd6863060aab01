"""The adversarial sets of tests/triangle_rotated.cpp as data -- shared by tests/test_triangle_exact.py (CPU) and
tests/test_gpu_triangle.py (device): the program's `--dump` mode, the shares the sets must have, and the exact evaluation of the
"exact zeros" set from its inputs alone."""
import os
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["random", "axis ties", "shared edges and vertices", "exact zeros", "double-precision fall-back", "denormal products", "interval ends"]
WORDS = 26          # 17 floats of the case | accepted a invDet U V W | enters the fall-back | RayAux::k of rayAux, of rayAuxRotated
ACCEPTED, A, INVDET, U, V, W, FALLBACK, K_SELECT, K_ROTATED = 17, 18, 19, 20, 21, 22, 23, 24, 25
RAY_FLIP = 0x80000000


def dump(directory, cases_per_set):
    """compiles the program as tests/test_triangle_rotated.py does and returns {set: uint32 [cases_per_set, 26]}"""
    exe, out = os.path.join(str(directory), "triangle_rotated"), os.path.join(str(directory), "cases.bin")
    subprocess.run(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "triangle_rotated.cpp"), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, "--dump", out, str(cases_per_set)], capture_output=True, timeout=600)
    assert r.returncode == 0 and "total: 0 differences" in r.stdout.decode(), r.stdout.decode() + r.stderr.decode()
    words = np.fromfile(out, dtype=np.uint32)
    os.remove(out)
    assert words.size == len(SETS) * cases_per_set * WORDS
    words = words.reshape(len(SETS), cases_per_set, WORDS)
    return {name: words[i] for i, name in enumerate(SETS)}


def is_nan(words):
    return (words & 0x7fffffff) > 0x7f800000


def is_nonfinite(words):
    return (words & 0x7f800000) == 0x7f800000


def is_denormal(words):
    return ((words & 0x7f800000) == 0) & ((words & 0x007fffff) != 0)


def shares(sets):
    """per set: share of cases with a NaN result word, with a non-finite one, share that enters the fall-back, share of ACCEPTED cases with a denormal
    U, V or W"""
    out = {}
    for name, w in sets.items():
        accepted = w[:, ACCEPTED] == 1
        out[name] = {"nan": float(is_nan(w[:, A:W + 1]).any(axis=1).mean()), "nonfinite": float(is_nonfinite(w[:, A:W + 1]).any(axis=1).mean()),
                     "fallback": float((w[:, FALLBACK] == 1).mean()),
                     "denormal": float(is_denormal(w[accepted][:, U:W + 1]).any(axis=1).mean()) if accepted.any() else 0.0,
                     "accepted": float(accepted.mean())}
    return out


def check_shares(sets):
    """what the sets must be for the comparisons to mean something; returns the shares for printing"""
    s = shares(sets)
    for name in SETS:
        assert s[name]["nan"] <= 0.10, (name, s[name])
        if name != "denormal products":
            assert s[name]["nan"] == 0.0, (name, s[name])
        assert s[name]["accepted"] > 1e-4, (name, s[name])
    assert s["double-precision fall-back"]["fallback"] > 0.5, s["double-precision fall-back"]
    assert s["denormal products"]["denormal"] >= 0.25, s["denormal products"]
    ends = sets["interval ends"]                    # both outcomes, at either end of the interval
    lower = ends[:, 16] == np.float32(3.402823466e+38).view(np.uint32)
    for side in (lower, ~lower):
        assert 0.2 < (ends[side][:, ACCEPTED] == 1).mean() < 0.8
    return s


# ---- the "exact zeros" set: small integers, directions scaled by powers of two, so every intermediate value of the test is
# ---- exact in any precision and the outcome follows from the inputs alone

def _axes(d):
    """the reference's choice of kz, kx, ky (hitable.hpp:78-98) for one direction"""
    ax, ay, az = abs(d[0]), abs(d[1]), abs(d[2])
    kz = 2 if (az >= ay and az >= ax) else (1 if ay >= ax else 0)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    return kx, ky, kz


def exact_case(f17):
    """One case in rational arithmetic (fractions): (accepted, U, V, W) by the reference's rule -- the sign tests, det == 0, the
    interval against T * sign(det) (hitable_triangle.hpp:219-262)."""
    x = [Fraction(float(v)) for v in f17]
    v0, v1, v2, o, d, amin, amax = x[0:3], x[3:6], x[6:9], x[9:12], x[12:15], x[15], x[16]
    kx, ky, kz = _axes(d)
    Sx, Sy, Sz = d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
    P = [[v[i] - o[i] for i in range(3)] for v in (v0, v1, v2)]
    (Ax, Ay), (Bx, By), (Cx, Cy) = [(p[kx] - Sx * p[kz], p[ky] - Sy * p[kz]) for p in P]
    Uv, Vv, Wv = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    if (Uv < 0 or Vv < 0 or Wv < 0) and (Uv > 0 or Vv > 0 or Wv > 0):
        return False, Uv, Vv, Wv
    det = Uv + Vv + Wv
    if det == 0:
        return False, Uv, Vv, Wv
    T = Uv * Sz * P[0][kz] + Vv * Sz * P[1][kz] + Wv * Sz * P[2][kz]
    s = -1 if det < 0 else 1
    if T * s < amin * det * s or T * s > amax * det * s:
        return False, Uv, Vv, Wv
    return True, Uv, Vv, Wv


def exact_set(words):
    """The whole set in numpy int64 -- integer arithmetic, exact: with dz = dir[kz] every sheared coordinate times dz is an
    integer, so U, V, W times dz^2 and T times dz^3 are.  Returns (accepted bool [n], U V W float64 [n, 3], exact: quotients of
    small integers by 1, 4 or 16).  exact_case() over a sample must agree with it (the tests check that)."""
    f = words[:, :17].view(np.float32).astype(np.float64)
    assert np.array_equal(f[:, :15], np.round(f[:, :15])) and np.abs(f[:, :15]).max() <= 4          # small integers
    assert (f[:, 15] == -np.float32(3.402823466e+38)).all() and (f[:, 16] == np.float32(3.402823466e+38)).all()
    i = f[:, :15].astype(np.int64)
    d = i[:, 12:15]
    ad = np.abs(d)
    kz = np.where((ad[:, 2] >= ad[:, 1]) & (ad[:, 2] >= ad[:, 0]), 2, np.where(ad[:, 1] >= ad[:, 0], 1, 0))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    n = np.arange(len(i))
    dz = d[n, kz]
    assert (dz != 0).all()
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    P = [i[:, 3 * c:3 * c + 3] - i[:, 9:12] for c in range(3)]
    x = [p[n, kx] * dz - d[n, kx] * p[n, kz] for p in P]      # Ax, Bx, Cx times dz
    y = [p[n, ky] * dz - d[n, ky] * p[n, kz] for p in P]
    Ui, Vi, Wi = x[2] * y[1] - y[2] * x[1], x[0] * y[2] - y[0] * x[2], x[1] * y[0] - y[1] * x[0]   # times dz^2 > 0
    mixed = ((Ui < 0) | (Vi < 0) | (Wi < 0)) & ((Ui > 0) | (Vi > 0) | (Wi > 0))
    det = Ui + Vi + Wi
    # the interval is (-FLT_MAX, FLT_MAX) times |det|, |det| >= 1/16 and |T| < 2^20: T * sign(det) lies inside it for every case
    Ti = Ui * P[0][n, kz] + Vi * P[1][n, kz] + Wi * P[2][n, kz]
    assert np.abs(Ti).max() < 1 << 40
    accepted = ~mixed & (det != 0)
    dz2 = (dz * dz).astype(np.float64)
    return accepted, np.stack([Ui / dz2, Vi / dz2, Wi / dz2], axis=1)


def assert_exact(words, accepted_words, uvw_words, label):
    """accepted flags (n) and U, V, W bits (n, 3) of some evaluation of the set against the exact one; the sign of a zero is not
    part of this comparison (the bitwise comparisons cover it)"""
    accepted, uvw = exact_set(words)
    assert 0.05 < accepted.mean() < 0.5 and (uvw[accepted] == 0).any(axis=1).mean() > 0.3     # corners and edges are common
    got = accepted_words == 1
    assert np.array_equal(got, accepted), (label, int((got != accepted).sum()))
    got_uvw = np.ascontiguousarray(uvw_words).view(np.float32).astype(np.float64)
    bad = (got_uvw[accepted] != uvw[accepted]).any(axis=1)
    assert not bad.any(), (label, int(bad.sum()))
