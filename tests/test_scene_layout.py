"""wpt_scene_layout.h: how a description becomes the arrays the kernels read, as pure host functions (no device).
tests/scene_layout_check.cpp compiles the header outside the library, without a header of HIP or of the kernels, with
-fsanitize=address,undefined, and is run as a program: it checks the layout of seeded random descriptions against what must hold
whatever the implementation, runs every layout function over damaged descriptions that validation still accepts, and prints the
digests that tests/golden/scene_layout_digests.json pins."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("nodes", "wide", "geometry", "attributes", "hotspots", "textures", "rgl_pool", "rgbl", "env_M", "env_Ms", "env_Mcs", "env_lut")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_layout") / "scene_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "scene_layout_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_layout_on_its_own_under_the_sanitizers(program):
    """storage order, links, boxesMayBeNan, triangle order, wide form, texel offsets, measured-BRDF tables and environment tables of
    random descriptions; validate() and then every layout function over at least 10^5 damaged ones; the new NULL checks"""
    r = subprocess.run([program], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-3000:]
    assert " 0 failures" in out and "BROKEN" not in out
    assert not r.stderr, r.stderr.decode()[-2000:]
    words = out.strip().splitlines()[-1].replace(";", " ").replace(",", " ").split()
    damaged, valid = int(words[words.index("damaged") - 1]), int(words[words.index("valid") - 3])
    assert damaged >= 100000 and valid >= damaged // 20, out


def test_the_arrays_are_the_recorded_ones(program):
    """a 64-bit FNV-1a of every array for six fixed descriptions, with 0, 7 and 65536 nodes in front and both triangle orders: a
    change to the layout is a deliberate edit of tests/golden/scene_layout_digests.json (profiles/scene_layout_digests.txt has the
    same digests beside those of the statements wpt_scene_upload held before the layout had a file of its own)"""
    r = subprocess.run([program, "--digests"], capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    got = {}
    for line in r.stdout.decode().splitlines():
        key, _, digest = line.rpartition(" ")
        assert key not in got
        got[key] = digest
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "scene_layout_digests.json")))
    assert len(golden) == 6 * 3 * 2 * len(ARRAYS)
    for seed in range(1, 7):
        for top in (0, 7, 65536):
            for order in ("leaves", "given"):
                for name in ARRAYS:
                    assert "seed %d top %d %s %s" % (seed, top, order, name) in golden
    assert "none" not in golden.values()        # every description has a wide form and a start table
    assert got == golden, sorted(k for k in golden if got.get(k) != golden[k])[:10]
    # the storage order shows where it should: the large tree's nodes differ with what goes in front, its triangles with their order
    assert len({golden["seed 6 top %d leaves nodes" % top] for top in (0, 7, 65536)}) == 3
    assert golden["seed 6 top 0 leaves geometry"] != golden["seed 6 top 0 given geometry"]


def test_digests_and_code_objects_are_recorded_unchanged():
    """profiles/scene_layout_digests.txt: every array is the parent's; profiles/scene_layout_code_objects.txt, written by
    tools/code_object_compare.sh: every translation unit compiles to the same gfx950 code object as before (wpt_capi among them:
    only its host side changed)"""
    rows = [line.split(" : ") for line in open(os.path.join(ROOT, "profiles", "scene_layout_digests.txt")) if not line.startswith("#")]
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "scene_layout_digests.json")))
    assert len(rows) == len(golden)
    for key, parent, this, verdict in rows:
        assert verdict.strip() == "same" and parent.strip() == this.strip() == golden[key.strip()], key
    rows = [line.split(" : ") for line in open(os.path.join(ROOT, "profiles", "scene_layout_code_objects.txt")) if not line.startswith("#")]
    verdict = {r[0]: r[-1].strip() for r in rows}
    assert len(verdict) == 46
    assert all(v == "same" for v in verdict.values()), verdict
    assert "wpt_capi" in verdict and "wpt_k_progress" in verdict and sum(u.startswith(("wpt_k_basic", "wpt_k_full")) for u in verdict) == 37


def test_upload_has_one_statement_of_the_node_record():
    """wpt_scene_upload keeps no layout of its own: no UP macro, and the node record's word order is written in one file"""
    csrc = os.path.join(ROOT, "wurblpt_amd", "csrc")
    units = sorted(n for n in os.listdir(csrc) if n == "wpt_capi_common.h" or (n.startswith("wpt_capi") and n.endswith(".hip")))
    assert "wpt_capi.hip" in units and "wpt_capi_scene.hip" in units and "wpt_capi_common.h" in units
    capi = "".join(open(os.path.join(csrc, n)).read() for n in units)
    layout = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "wpt_scene_layout.h")).read()
    assert "define UP" not in capi and "hip_runtime" not in layout
    assert "nd.lo[0], nd.hi[0], nd.lo[1], nd.lo[2]" in layout and "nd.lo[0], nd.hi[0]" not in capi
    assert "g_walk" not in layout and "g_topNodes" not in layout
