"""Inner nodes whose children's boxes lie within their own are left out of the walk of a tree in LDS
(wurblpt_amd/csrc/wpt_bypass.h): a ray that fails such a node's box fails its children's, so every link that led to the node
leads to its first child.  CPU tests of the code wpt_scene_upload runs: tests/bypass_walk.cpp walks random trees under the real
slab arithmetic with bounds that move, next to the reference's walk (the same leaves under the same bounds, exactly the visits
to left-out nodes saved minus the extra failing tests, wrong rules caught), and the Cornell box's own plan is walked here on
rays of the scene next to the oracle's BVH::hit."""
import os
import subprocess
import time

import numpy as np

from wurblpt_amd import device, host
from tests.test_fold_walk import scene_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
INNER, TRIANGLE, EMPTY = 0, 1, 3   # wpt_bvh_node::kind


def test_walks_of_random_trees_with_nodes_left_out(tmp_path):
    exe = str(tmp_path / "bypass_walk")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "bypass_walk.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert "trees 3000, walks 384000" in out, out
    assert "cases covered: yes" in out, out
    assert "model plans with more visits on their sample than the fold: 0" in out, out
    assert "ineligible nodes left out: 0" in out, out
    assert "differ from the model's closed form: 0 " in out, out
    assert "plan of a tree of 577 nodes, 40 triangles (20384 bytes in LDS)" in out, out
    assert "walks that differ: 0" in out, out


def left_out(links, start, kind):
    """the inner nodes no link of the plan leads to"""
    n = len(links)
    targets = {int(start)} | {int(s) for s in links[:, 0]} | {int(w) for w in links[:, 1] if w < 1 << 31}
    return [i for i in range(n) if kind[i] == INNER and i not in targets]


def test_the_cornell_boxs_plan(oracle):
    """The bench scene's tree.  As in tests/test_fold_walk.py every ray walks under one bound from the root on, so that the box
    decisions are a table of (ray, node) from the oracle's AABB::mayHit: once under the bound its walk ends with, where the plain
    walk over the table must visit exactly the nodes the oracle's BVH::hit counts, and once under the open bound.  Over both
    tables the walk over the plan's links tests the leaves of the plain walk in its order, and saves at least a fifth of the
    folded walk's visits (the issue's greedy optimum on these rays: 25 - 27 %)."""
    sc = host.cornell(64, 64, 1, 2)
    nodes = sc.nodes_array()
    n = len(nodes)
    assert n == 71 and int(sc.d.tri_count) == 36
    folded_count, folded = device.fold_plan(sc, with_words=True)
    count, links, start = device.bypass_plan(sc, with_words=True)
    count2, links2, start2 = device.bypass_plan(sc, with_words=True)
    assert (count, start) == (count2, start2) and np.array_equal(links, links2)   # same scene, same plan
    assert folded_count == 6 and device.fold_plan(sc) == 6                         # the fold's plan keeps its meaning
    kind, link = nodes[:, 7], nodes[:, 6]
    gone = left_out(links, start, kind)
    print("left out: %d nodes; no link leads to %s; rays start at node %d" % (count, gone, start))
    assert count > 0 and start != 0 and 0 in gone                                  # the root is left out
    end = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        end[i] = end[link[i]] if kind[i] == INNER else i + 1
    for i in range(n):
        if kind[i] == TRIANGLE:
            assert links[i, 1] == folded[i] == (~int(link[i])) & 0xffffffff
    boxes = nodes[:, :6].copy()

    rays = scene_rays(oracle, sc, 2048, 6144, 5)
    first, _ = oracle.bvh_hits(sc, rays)
    rays = rays[first[:, 0] > 0]
    first = first[first[:, 0] > 0]
    m = len(rays)
    assert m > 4000
    for bound in ("final", "open"):
        if bound == "final":
            rays[:, 7] = first[:, 2]
            _, counters = oracle.bvh_hits(sc, rays)
        else:
            rays[:, 7] = np.float32(FLT_MAX)
        table = oracle.simple("wpt_oracle_aabb", m * n, 1, np.tile(boxes.view(np.float32), (m, 1)), np.repeat(rays, n, axis=0),
                              out_dtype=np.int32).reshape(m, n) != 0
        plain_visits = folded_visits = plan_visits = leaf_tests = 0
        for r in range(m):
            hit = table[r]
            seq_plain, seq_folded, seq_plan = [], [], []
            node = 0
            while node < n:
                plain_visits += 1
                if hit[node] and kind[node] == INNER:
                    node += 1
                else:
                    if hit[node] and kind[node] == TRIANGLE:
                        seq_plain.append(int(link[node]))
                    node = end[node]
            node = 0
            while node < n:
                folded_visits += 1
                w = int(folded[node])
                if hit[node] and w >= 1 << 31:
                    seq_folded.append((~w) & 0xffffffff)
                    node = end[node]
                else:
                    node = w if hit[node] else end[node]
            node = start
            while node < n:
                plan_visits += 1
                w = int(links[node, 1])
                if hit[node] and w >= 1 << 31:
                    seq_plan.append((~w) & 0xffffffff)
                    node = int(links[node, 0])
                else:
                    node = w if hit[node] else int(links[node, 0])
            assert seq_plain == seq_folded == seq_plan, r
            leaf_tests += len(seq_plain)
        saved = 1.0 - plan_visits / folded_visits
        print("%s bound, %d rays: node visits per ray %.2f plain, %.2f folded, %.2f with the plan (%.1f %% of the folded walk's saved); leaf tests per ray %.2f"
              % (bound, m, plain_visits / m, folded_visits / m, plan_visits / m, 100.0 * saved, leaf_tests / m))
        if bound == "final":
            assert plain_visits == counters["node_visits"] and leaf_tests == counters["leaf_tests"]
        assert saved >= 0.20, saved


def test_every_eligible_node_and_the_time_of_a_plan():
    """wpt_set_bypass(1) leaves every eligible node out (the Cornell tree is nested: all inner nodes but those the links still
    need), and the plan of the largest tree of triangles alone that fits LDS (365 nodes) takes a bounded time.  (640 nodes of
    32 bytes leave no room for a triangle; tests/bypass_walk.cpp times 577 nodes with 40 triangles, all inner nodes eligible.  The
    search is at most 8 passes over the eligible nodes with one O(nodes) evaluation each.)"""
    sc = host.cornell(64, 64, 1, 2)
    model = device.bypass_plan(sc)
    try:
        device.set_bypass(device.BYPASS_ALL_ELIGIBLE)
        everything = device.bypass_plan(sc)
    finally:
        device.set_bypass(device.BYPASS_MODEL)
    inner = int((sc.nodes_array()[:, 7] == INNER).sum())
    assert model < everything <= inner and device.bypass_plan(sc) == model
    for triangles in range(183, 170, -1):   # 183 triangles, 365 nodes: the largest tree of triangles that fits (the scene adds a few)
        big = host.random_triangles(triangles, 7, 33, 33, with_texcoords=False)
        if big.d.node_count * 32 + big.d.tri_count * 48 <= 20 * 1024:
            break
    assert big.d.node_count * 32 + big.d.tri_count * 48 <= 20 * 1024 and big.d.node_count >= 341
    t0 = time.perf_counter()
    count = device.bypass_plan(big)
    seconds = time.perf_counter() - t0
    print("plan of a tree of %d nodes, %d triangles: %d nodes left out, %.1f ms" % (big.d.node_count, big.d.tri_count, count, 1e3 * seconds))
    assert seconds < 5.0
