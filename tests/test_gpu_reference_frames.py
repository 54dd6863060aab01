"""The product's mcpt() on the MI355X against frames rendered by the reference's own mcpt().

tests/golden/frames/ holds what oracle/ref_frames.cpp wrote: the reference's whole library, compiled where its tree exists, over the
cases of oracle/pin_scenes.hpp (every material, spot lights, textures, environment maps, spheres, hot spots, measured BRDFs, key
frames, lens, gates, the integrator's parameters, a Cornell box, the time-of-flight sensor).  Here oracle/pin_render.cpp, the same
cases compiled against include/ and linked to libwurblpt_hip.so, renders them once per module with the product's mcpt(); every
frame must be the reference's bit for bit.  The same program gives the reference's hit vectors (vectors_hits_*.npy: rays through
edges, corners and planes with the records of Scene::bvh().hit) to the device's own walk, triangle test and finishHit through the
test hook wpt_selftest_hits; every column but the triangle's index must be the reference's bits.  Only tests/golden/ is read,
never the reference."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAMES = os.path.join(GOLDEN, "frames")

with open(os.path.join(FRAMES, "index.json")) as _f:
    CASES = json.load(_f)["cases"]
NAMES = [c["name"] for c in CASES]
HIT_VECTORS = sorted(f[:-4] for f in os.listdir(FRAMES) if f.startswith("vectors_hits_"))


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pin_device")
    exe = str(tmp / "pin_render")
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-DPIN_DEVICE", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "oracle", "pin_render.cpp"), "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-ldl", "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    out = tmp / "frames"
    out.mkdir()
    r = subprocess.run([exe, GOLDEN, str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return out


def differing(a, b):
    assert a.shape == b.shape and a.dtype == np.float32 and b.dtype == np.float32
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def test_every_case_was_rendered(rendered):
    assert len(NAMES) >= 30 and any(c["tof"] for c in CASES)
    assert sorted(f[:-4] for f in os.listdir(rendered) if f.endswith(".npy")) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_frame_is_the_references(rendered, name):
    got, ref = np.load(rendered / (name + ".npy")), np.load(os.path.join(FRAMES, name + ".npy"))
    assert np.isfinite(got).all()
    n = differing(got, ref)
    assert n == 0, "%s: %d of %d floats differ from the reference's frame (means %.6g / %.6g)" % (name, n, ref.size, got.mean(), ref.mean())


def test_the_hit_vectors_are_all_answered(rendered):
    assert {"vectors_hits_cornell", "vectors_hits_textures"} <= set(HIT_VECTORS)
    assert sorted(f[:-4] for f in os.listdir(rendered / "vectors")) == HIT_VECTORS


@pytest.mark.parametrize("name", HIT_VECTORS)
def test_device_hit_records_are_the_references(rendered, name):
    """8 floats of the ray | haveHit, triangle, a, position, normal, tangent, texcoords, backside"""
    got, ref = np.load(rendered / "vectors" / (name + ".npy")), np.load(os.path.join(FRAMES, name + ".npy"))
    assert ref.shape[1] == 23 and len(ref) >= 64 and 0.3 < ref[:, 8].mean() < 1.0 and np.isfinite(ref).all()
    assert got.shape == ref.shape
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d rows differ, in columns %s" % (name, bad.any(axis=1).sum(), np.nonzero(bad.any(axis=0))[0].tolist())
