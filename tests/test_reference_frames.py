"""The CPU restatement (oracle/) against frames rendered by the reference's own mcpt().

tests/golden/frames/ holds what oracle/ref_frames.cpp wrote: the reference's whole library, compiled where its tree exists (with the
container stand-in oracle/tgd_standin/), over the cases of oracle/pin_scenes.hpp.  Here oracle/pin_render.cpp -- the same cases
compiled against include/ -- flattens every scene and renders it with wpt_oracle_render of both math back ends; every frame must be
the reference's bit for bit, no pixel left out and no tolerance.  Vectors of the reference's own classes (materials, hot spots,
environment maps, the triangle test) go through the restatement's probes the same way, and the time-of-flight sensor's
accumulation through the product's host rule.  Where the reference's tree exists, its program is run again and must reproduce the committed
fixtures byte for byte."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAMES = os.path.join(GOLDEN, "frames")
REF_FRAMES = os.path.join(ROOT, "oracle", "_ref", "ref_frames")

with open(os.path.join(FRAMES, "index.json")) as _f:
    INDEX = json.load(_f)
CASES = INDEX["cases"]
BY_NAME = {c["name"]: c for c in CASES}
RGB = [c["name"] for c in CASES if not c["tof"]]
TOF = [c["name"] for c in CASES if c["tof"]]
BACKENDS = {"portable": "liboracle.so", "libm": "liboracle_libm.so"}
# vectors of the reference's classes that the restatement answers (the time-of-flight ones go to the product's host rule)
VECTORS = sorted(f[:-4] for f in os.listdir(FRAMES) if f.startswith("vectors_") and f != "vectors_tof_accumulate.npy")

# what the issue asks the table of cases to carry; a case that is dropped from oracle/pin_scenes.hpp fails here
REQUIRED_FEATURES = ["lambertian", "light_diffuse", "ggx", "glass", "mirror", "modphong", "opacity", "twosided", "spot", "checker",
                     "transformer", "image_u8", "image_u16", "image_f32", "normalmap", "envmap_equirect", "importance", "envmap_cube",
                     "sphere", "sphere_hotspot", "hotspots", "rgl", "animation", "camera_animation", "thinlens", "distortion", "gate",
                     "max_path_components", "roulette_off", "pixel_centres", "cornell", "shared_edges", "tof", "light_tof"]


def golden_frame(name):
    return np.load(os.path.join(FRAMES, name + ".npy"))


def differing(a, b):
    assert a.shape == b.shape and a.dtype == np.float32 and b.dtype == np.float32, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """oracle/pin_render.cpp compiled once against include/; it loads the restatement library it is given, so one program serves
    both back ends.  It writes every case's frame and, in the fixtures' layout, the restatement's answers to the vector files"""
    tmp = tmp_path_factory.mktemp("pin_oracle")
    exe = str(tmp / "pin_render")
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "oracle", "pin_render.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    dirs = {}
    for backend, lib in BACKENDS.items():
        out = tmp / backend
        out.mkdir()
        r = subprocess.run([exe, os.path.join(ROOT, "oracle", lib), GOLDEN, str(out)], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        dirs[backend] = out
    return dirs


# ---- the fixtures themselves: conditions on the reference's frames alone ----

def test_the_table_of_cases_is_complete():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    features = set(f for c in CASES for f in c["features"])
    assert [f for f in REQUIRED_FEATURES if f not in features] == []
    for c in CASES:
        assert os.path.exists(os.path.join(FRAMES, c["name"] + ".npy")), c["name"]
        assert all(u in BY_NAME for u in c["unlike"]), c
    # every .npy in the directory is a case of the index or one of the vector files: nothing escapes the comparison
    files = sorted(f[:-4] for f in os.listdir(FRAMES) if f.endswith(".npy"))
    assert [f for f in files if f not in BY_NAME and not f.startswith("vectors_")] == []
    # the spot lights: cones of 30, 70 and 360 degrees, with and without a texture, and inside a two-sided material
    spot = {n: c for n, c in BY_NAME.items() if "spot" in c["features"]}
    assert {"spot_30", "spot_70", "spot_360"} <= set(spot)
    assert any("checker" in c["features"] for c in spot.values()) and any("twosided" in c["features"] for c in spot.values())
    for n, c in spot.items():
        assert "spot_none" in c["unlike"], n                   # differs from the same scene without the lamp
        if "360" not in n:
            assert any("360" in u for u in c["unlike"]), n       # a partial cone differs from its full-circle twin
    for n, c in BY_NAME.items():
        if "gate" in c["features"]:
            assert "ggx" in c["unlike"], n                      # a gated frame differs from the ungated one


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_reference_frame_is_finite_and_lit(name):
    c = BY_NAME[name]
    f = golden_frame(name)
    assert f.dtype == np.float32
    assert f.shape == ((4, c["height"], c["width"], 3) if c["tof"] else (c["height"], c["width"], 3))
    assert np.isfinite(f).all()
    for plane in (f if c["tof"] else [f]):
        lit = (plane.reshape(-1, 3) != 0).any(axis=1)
        assert lit.mean() >= 0.5, (name, lit.mean())
    assert os.path.getsize(os.path.join(FRAMES, name + ".npy")) < 64 * 1024


def test_reference_frames_that_must_differ_do():
    pairs = [(c["name"], u) for c in CASES for u in c["unlike"]]
    assert len(pairs) >= 30
    for a, b in pairs:
        assert differing(golden_frame(a), golden_frame(b)) > 0, (a, b)


def test_the_four_tof_phases_differ_pairwise():
    assert TOF
    for name in TOF:
        f = golden_frame(name)
        for i in range(4):
            for j in range(i):
                assert differing(f[i], f[j]) > 0, (name, i, j)
            # a + b = total up to rounding, and the modulated part moves energy between the taps
            assert np.allclose(f[i][..., 0] + f[i][..., 1], f[i][..., 2], rtol=1e-5)


# ---- the restatement against the reference ----

def test_no_case_is_left_out(rendered):
    for backend, out in rendered.items():
        got = sorted(f[:-4] for f in os.listdir(out) if f.endswith(".npy"))
        assert got == sorted(RGB + VECTORS), backend
    assert len(RGB) >= 30


@pytest.mark.parametrize("backend", sorted(BACKENDS))
@pytest.mark.parametrize("name", RGB)
def test_restatement_frame_is_the_references(rendered, name, backend):
    got, ref = np.load(rendered[backend] / (name + ".npy")), golden_frame(name)
    n = differing(got, ref)
    assert n == 0, "%s (%s): %d of %d floats differ from the reference's frame (means %.6g / %.6g)" % (name, backend, n, ref.size, got.mean(), ref.mean())


# ---- vectors of the reference's own classes through the restatement's probes ----

def test_the_vectors_reach_what_they_are_for():
    assert {"vectors_materials", "vectors_hits_cornell"} <= set(VECTORS)
    assert sum(v.startswith("vectors_hotspots_") for v in VECTORS) >= 2 and sum(v.startswith("vectors_envmap_") for v in VECTORS) >= 2
    m = np.load(os.path.join(FRAMES, "vectors_materials.npy"))       # material index | 18 in | 22 out
    assert m.shape[1] == 41 and len(np.unique(m[:, 0])) >= 20
    assert {0.0, 1.0, 2.0} <= set(np.unique(m[:, 19]))                # no scattering, explicit and random directions
    emits = np.array([m[m[:, 0] == k][:, 37:41].any(axis=1).mean() for k in np.unique(m[:, 0])])
    assert ((emits > 0) & (emits < 0.5)).sum() >= 4                   # lights with a cone: some rays inside it, most outside
    tof = m[(m[:, 37:40] == 0).all(axis=1) & (m[:, 40] > 0)]           # ToF lights emit in the fourth channel only,
    assert len(np.unique(tof[:, 0])) == 2 and len(np.unique(tof[:, 40])) > 2   # plain and scaled by a texture's red value
    h = np.load(os.path.join(FRAMES, "vectors_hits_cornell.npy"))     # 8 in | 15 out
    assert h.shape[1] == 23 and 0.5 < h[:, 8].mean() < 1.0 and h[:, 22].any()
    assert (h[:, 4] == 0).sum() >= 48                                 # rays that travel in a plane of the room
    for v in VECTORS:
        if v.startswith("vectors_hotspots_"):
            r = np.load(os.path.join(FRAMES, v + ".npy"))             # 7 in | 7 out
            assert r.shape[1] == 14 and (r[:, 7] > 0).mean() > 0.3 and (r[:, 12] > 0).mean() > 0.9
        if v.startswith("vectors_envmap_"):
            r = np.load(os.path.join(FRAMES, v + ".npy"))             # 4 in | 10 out
            assert r.shape[1] == 14 and (r[:, 8] > 0).all() and r[:, 8].max() > 4 * r[:, 8].min()
    assert all(os.path.getsize(os.path.join(FRAMES, v + ".npy")) < 128 * 1024 for v in VECTORS)


@pytest.mark.parametrize("backend", sorted(BACKENDS))
@pytest.mark.parametrize("name", VECTORS)
def test_restatement_answers_as_the_references_classes_do(rendered, name, backend):
    got, ref = np.load(rendered[backend] / (name + ".npy")), np.load(os.path.join(FRAMES, name + ".npy"))
    assert np.isfinite(ref).all()
    bad = (got.view(np.uint32) != ref.view(np.uint32))
    assert got.shape == ref.shape and not bad.any(), "%s (%s): %d rows differ, in columns %s" % (
        name, backend, bad.any(axis=1).sum(), np.nonzero(bad.any(axis=0))[0].tolist())


# ---- the time-of-flight rule of the product (one header for the kernels and the host) against the reference's sensor ----

def test_tof_accumulation_is_the_references():
    """rows of [radiance.w, opl.w, isTofLight, phase, a, b, total] from SensorTofAmcw::accumulateRadiance with the sensor's defaults"""
    rows = np.load(os.path.join(FRAMES, "vectors_tof_accumulate.npy"))
    assert rows.shape[1] == 7 and rows.shape[0] >= 256
    assert set(rows[:, 3].astype(int)) == {0, 1, 2, 3} and set(rows[:, 2].astype(int)) == {0, 1}
    sensor = host.tof_sensor()      # SensorTofAmcw's defaults, as the reference's sensor has them
    assert sensor.phase_count == 4
    got = np.zeros((rows.shape[0], 3), dtype=np.float32)
    for i, r in enumerate(rows):
        got[i] = device.tof_accumulate_host(sensor, int(r[3]), float(r[0]), float(r[1]), int(r[2]), np.zeros(3, dtype=np.float32))
    assert differing(got, np.ascontiguousarray(rows[:, 4:7])) == 0
    modulated = rows[(rows[:, 2] == 1) & (rows[:, 0] > 0)]
    assert (modulated[:, 4] != modulated[:, 5]).mean() > 0.9   # the vectors do exercise the cosine


# ---- the fixtures are what the reference writes today ----

@pytest.mark.skipif(not os.path.exists(REF_FRAMES), reason="the reference's tree is not on this machine (oracle/_ref/ref_frames is not built)")
def test_reference_program_reproduces_the_fixtures(tmp_path):
    r = subprocess.run([REF_FRAMES, GOLDEN, str(tmp_path)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    committed, fresh = sorted(os.listdir(FRAMES)), sorted(os.listdir(tmp_path))
    assert committed == fresh
    match, mismatch, errors = filecmp.cmpfiles(FRAMES, str(tmp_path), committed, shallow=False)
    assert mismatch == [] and errors == []
