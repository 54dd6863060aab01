"""The large form of the kernel with rotated corners walks ordered box copies: the node array once per sign octant of a ray's
direction, mirrored on the negative axes, so that a box test sorts no slab distances (wurblpt_amd/csrc/wpt_scene_layout.h,
orderedBoxCopies; wpt_device.h, boxTestOrdered).  CPU tests of the code wpt_scene_upload runs and of the test's arithmetic:
tests/ordered_boxes.cpp compares the verdicts of the ordered test with boxTest's for 10^7 random and for adversarial pairs,
checks the copies of random trees, of the tree that fills LDS and of the scenes' trees written to files here, and walks a
model with the ordered step next to the model with the present one.  The same program runs once more under the host
sanitizers.  The scenes that tests/test_gpu_ordered_boxes.py renders in the large form must qualify for it: the bench scene
first of all."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import device, host

from tests import lds_edge_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, TRIANGLE = 0, 1   # wpt_bvh_node::kind
NODE_CHILD = 0xc0000000
LARGE_COLD_BYTES = 512 + 8 * 1024 * 16    # the tables and the cold words of 1024 lanes
LDS_BYTES_PER_CU = 160 * 1024
EDGE_SCENES = [(16, 34), (32, 8), (36, 2)]


def large_request(node_count, scene_lds_bytes):
    """the LDS bytes a launch in the large form needs (wpt_pathtrace.inc.h, orderedPlaces): copy k >= 1 of the node array lies at
    base + k * stride quadwords, behind the scene, base a multiple of 16 and stride 2 more than one"""
    node_quads = 2 * node_count + 2
    used = scene_lds_bytes // 16
    stride = ((node_quads + 13) & ~15) + 2
    base = ((used - stride + 15) & ~15) if used > stride else 0
    return LARGE_COLD_BYTES + 16 * (base + 8 * stride)


def tree_file(sc, path):
    """the device words of a small scene's tree (nodes in depth-first order) and its triangle records, as tests/leaf_words.cpp
    loads them"""
    nodes = sc.nodes_array()
    n, m = len(nodes), int(sc.d.tri_count)
    kind, link = nodes[:, 7], nodes[:, 6]
    end = np.zeros(n + 1, np.int64)
    for i in range(n - 1, -1, -1):
        end[i] = end[link[i]] if kind[i] == INNER else i + 1
    words = np.zeros((n, 8), np.uint32)
    lo, hi = nodes[:, 0:3], nodes[:, 3:6]
    words[:, 0], words[:, 1], words[:, 2], words[:, 3], words[:, 4], words[:, 5] = lo[:, 0], hi[:, 0], lo[:, 1], lo[:, 2], hi[:, 1], hi[:, 2]
    for i in range(n):
        words[i, 6] = end[i]
        words[i, 7] = (NODE_CHILD | (i + 1)) if kind[i] == INNER else int(link[i]) if kind[i] == TRIANGLE else (NODE_CHILD | int(end[i]))
    with open(path, "wb") as f:
        f.write(np.array([n, m], np.uint32).tobytes())
        f.write(words.tobytes())
        f.write(C.string_at(sc.d.tri_geom, 48 * m))


def scenes():
    return [("cornell", host.cornell(64, 64, 1, 2))] + [("edge_%d_%d" % tm, cases.scene(*tm)) for tm in EDGE_SCENES]


def run(exe, pairs, files):
    r = subprocess.run([exe, str(pairs)] + files, capture_output=True, timeout=600)
    out = r.stdout.decode() + r.stderr.decode()
    print(out)
    assert r.returncode == 0, out
    assert "differing verdicts: 0" in out and "differing distances: 0" in out, out
    assert "71 nodes, 36 triangles, ordered copies" in out, out
    assert out.count(", ordered copies") == len(files) and "NO ordered copies" not in out, out
    assert "wrong 0;" in out and "not refused 0" in out, out
    assert "trees %d (%d from files)" % (301 + len(files), len(files)) in out, out
    assert "(30 without copies)" in out, out
    assert "walks that differ: 0" in out, out
    assert "cases covered: yes" in out, out
    return out


def write_trees(tmp_path):
    files = []
    for name, sc in scenes():
        files.append(str(tmp_path / (name + ".tree")))
        tree_file(sc, files[-1])
    return files


def test_ordered_test_and_copies_against_the_present_test(tmp_path):
    exe = str(tmp_path / "ordered_boxes")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "ordered_boxes.cpp"), "-o", exe], check=True, timeout=300)
    out = run(exe, 10 ** 7, write_trees(tmp_path))
    pairs = int(out.split("random pairs ")[1].split()[0])
    assert pairs >= 10 ** 7


def test_ordered_boxes_under_the_host_sanitizers(tmp_path):
    """the layout function and its check as a program of their own, built with the address and undefined-behaviour sanitizers
    (fewer random pairs: the instrumented program is slow)"""
    exe = str(tmp_path / "ordered_boxes_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "ordered_boxes.cpp"), "-o", exe], check=True, timeout=300)
    run(exe, 10 ** 5, write_trees(tmp_path))


@pytest.mark.parametrize("name,sc", scenes(), ids=[name for name, _ in scenes()])
def test_the_scenes_rendered_in_the_large_form_qualify(name, sc):
    """every box has lo <= hi (which no NaN passes), the kernel with rotated corners is the choice, and the request of a
    workgroup of 1024 lanes with the seven more node arrays, placed as orderedPlaces says, fits a compute unit's LDS"""
    nodes = sc.nodes_array().view(np.float32)
    lo, hi = nodes[:, 0:3], nodes[:, 3:6]
    assert (lo <= hi).all(), name
    if name == "cornell":
        d = sc.d
        chosen = device.kernel_choice(cases.GGX | cases.GLASS, device.SENSOR_FRAME, False, d.node_count, d.tri_count, d.material_count, False, 0, 0)
    else:
        chosen = cases.choice(sc, device.SENSOR_FRAME)
    assert chosen[1] == "rotated corners", (name, chosen)
    request = large_request(sc.d.node_count, chosen[3])
    print("%s: %d nodes, %d triangles, a request of %d bytes" % (name, sc.d.node_count, sc.d.tri_count, request))
    assert request <= LDS_BYTES_PER_CU, (name, request)
    if name == "cornell":
        assert request == 155648     # 131 584 + 16 * (336 + 8 * 146)
