"""The leaf pass of the kernels with rotated corner copies reads a leaf's triangle and skip links from the triangle's corner
records instead of the leaf's node (wurblpt_amd/csrc/wpt_leaf_words.h).  CPU tests of the code wpt_scene_upload runs:
tests/leaf_words.cpp checks the words of random trees, of a tree that fills LDS and of the Cornell box's tree (written to a
file here) under the plain, the folded and the bypass links, walks a model that takes them from the records next to the
model that reads the node, and wants the verdict "not one to one" for two hand-made trees.  The same program runs once more
under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np

from wurblpt_amd import device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, TRIANGLE, EMPTY = 0, 1, 3   # wpt_bvh_node::kind
NODE_CHILD = 0xc0000000


def cornell_tree(path):
    """the device words of the bench scene's tree as wpt_scene_layout.h makes them for a tree this small (nodes in depth-first
    order), with the triangle records in the caller's order, as wpt_fold_plan and wpt_bypass_plan take them"""
    sc = host.cornell(64, 64, 1, 2)
    nodes = sc.nodes_array()
    n, m = len(nodes), int(sc.d.tri_count)
    assert (n, m) == (71, 36)
    kind, link = nodes[:, 7], nodes[:, 6]
    end = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        end[i] = end[link[i]] if kind[i] == INNER else i + 1
    leaves = [i for i in range(n) if kind[i] == TRIANGLE]
    assert sorted(int(link[i]) for i in leaves) == list(range(m))      # one leaf per triangle
    words = np.zeros((n, 8), np.uint32)
    lo, hi = nodes[:, 0:3], nodes[:, 3:6]
    words[:, 0], words[:, 1], words[:, 2], words[:, 3], words[:, 4], words[:, 5] = lo[:, 0], hi[:, 0], lo[:, 1], lo[:, 2], hi[:, 1], hi[:, 2]
    for i in range(n):
        words[i, 6] = end[i]
        words[i, 7] = (NODE_CHILD | (i + 1)) if kind[i] == INNER else int(link[i]) if kind[i] == TRIANGLE else (NODE_CHILD | int(end[i]))
    # the library's own words for these leaves: a leaf's word in LDS is its triangle's index, complemented
    _, folded = device.fold_plan(sc, with_words=True)
    for i in leaves:
        assert int(folded[i]) == (~int(words[i, 7])) & 0xffffffff
    geom = C.string_at(sc.d.tri_geom, 48 * m)
    with open(path, "wb") as f:
        f.write(np.array([n, m], np.uint32).tobytes())
        f.write(words.tobytes())
        f.write(geom)


def run(exe, tree):
    r = subprocess.run([exe, tree], capture_output=True, timeout=300)
    out = r.stdout.decode() + r.stderr.decode()
    print(out)
    assert r.returncode == 0, out
    assert "71 nodes, 36 triangles" in out, out
    assert "trees 302 (1 from files, 30 with a NaN bound)" in out, out
    assert "wrong words: 0" in out and "wrong verdicts: 0" in out, out
    assert "hand-made trees judged not one to one: 2 of 2" in out, out
    assert "indices beyond the word refused: yes" in out, out
    assert "cases covered: yes" in out, out
    assert "walks that differ: 0" in out, out


def test_leaf_words_of_random_trees_and_the_cornell_box(tmp_path):
    exe, tree = str(tmp_path / "leaf_words"), str(tmp_path / "cornell.tree")
    cornell_tree(tree)
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "leaf_words.cpp"), "-o", exe], check=True, timeout=300)
    run(exe, tree)


def test_leaf_words_under_the_host_sanitizers(tmp_path):
    """the header and its check as a program of their own, built with the address and undefined-behaviour sanitizers"""
    exe, tree = str(tmp_path / "leaf_words_san"), str(tmp_path / "cornell.tree")
    cornell_tree(tree)
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "leaf_words.cpp"), "-o", exe], check=True, timeout=300)
    run(exe, tree)
