"""First children that repeat their parent's box are folded out of the tree's copy in LDS (wurblpt_amd/csrc/wpt_fold.h): their box
test repeats the parent's on the same inputs.  CPU tests of the rule the kernels' prologue and wpt_scene_upload run:
tests/fold_walk.cpp walks random trees folded and unfolded under a bound-dependent box predicate (the same leaves in the same
order, and exactly the visits to folded children saved), and the Cornell box's own tree is folded by the library and walked here
on rays of the scene next to the oracle's BVH::hit."""
import os
import subprocess

import numpy as np

from wurblpt_amd import device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
INNER, TRIANGLE, EMPTY = 0, 1, 3   # wpt_bvh_node::kind


def test_folded_and_unfolded_walks_of_random_trees(tmp_path):
    exe = str(tmp_path / "fold_walk")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "fold_walk.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert "trees 3000, walks 144000" in out, out
    assert "cases covered: yes" in out, out
    assert "walks that differ: 0" in out, out


def scene_rays(oracle, sc, n_camera, n_bounce, seed):
    """camera rays over the frame, and rays that leave the surfaces those hit in uniformly random directions: (n, 8) float32
    (origin, direction, amin, amax = FLT_MAX)"""
    rng = np.random.RandomState(seed)
    pq = rng.uniform(0.0, 1.0, (n_camera, 2)).astype(np.float32)
    cam = oracle.camera_rays(sc.camera.contents, pq).reshape(-1, 6)
    rays = np.concatenate([cam, np.full((n_camera, 1), 1e-4, np.float32), np.full((n_camera, 1), FLT_MAX, np.float32)], axis=1).astype(np.float32)
    hits, _ = oracle.bvh_hits(sc, rays)
    on = hits[hits[:, 0] > 0][:, 3:6]
    assert len(on) > n_camera // 2
    origins = on[rng.randint(0, len(on), n_bounce)]
    d = rng.normal(size=(n_bounce, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bounce = np.concatenate([origins, d, np.full((n_bounce, 1), 1e-4), np.full((n_bounce, 1), FLT_MAX)], axis=1).astype(np.float32)
    return np.concatenate([rays, bounce]).astype(np.float32)


def test_the_cornell_boxs_tree(oracle):
    """The bench scene's tree: the links the library folds, and the node visits that saves.  Every ray walks under the bound its
    walk ends with (its hit's distance from a first BVH::hit, given as amax), so the bound is one value from the root on: the box
    decisions are then a table of (ray, node) from the oracle's AABB::mayHit, the unfolded walk over that table must visit exactly
    as many nodes as the oracle's BVH::hit counts for the same rays, and the folded walk over the library's LDS words must test
    the same leaves and save exactly the visits to folded children."""
    sc = host.cornell(64, 64, 1, 2)
    nodes = sc.nodes_array()
    n = len(nodes)
    assert n == 71 and int(sc.d.tri_count) == 36
    inner, words = device.fold_plan(sc, with_words=True)
    print("folded nodes: %d" % inner)
    # counted on this tree: 6 inner nodes have an inner first child with their own box (the quads of floor, ceiling and walls; two
    # chains of two among them)
    assert inner == 6

    kind, link = nodes[:, 7], nodes[:, 6]
    end = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        end[i] = end[link[i]] if kind[i] == INNER else i + 1
    boxes = nodes[:, :6].copy()
    same_as_parent = [False] * n            # first children whose six bounds are their parent's, bit for bit
    for i in range(n):
        if kind[i] == INNER and np.array_equal(boxes[i], boxes[i + 1]):
            same_as_parent[i + 1] = True
    assert sum(1 for i in range(1, n) if same_as_parent[i] and kind[i] == INNER) == inner   # (a child has one parent)
    # the library's words: an index where a ray that passes the box goes; a leaf's word is its triangle complemented
    for i in range(n):
        if kind[i] == TRIANGLE:
            assert words[i] == (~int(link[i])) & 0xffffffff
        elif kind[i] == EMPTY:
            assert words[i] <= n
        else:
            c = i + 1
            while same_as_parent[c] and kind[c] == INNER:
                c += 1
            assert words[i] == c, (i, words[i], c)

    rays = scene_rays(oracle, sc, 1024, 3072, 5)
    first, _ = oracle.bvh_hits(sc, rays)
    rays[:, 7] = np.where(first[:, 0] > 0, first[:, 2], np.float32(FLT_MAX))
    bounded, counters = oracle.bvh_hits(sc, rays)
    # under its own bound a ray finds its hit again, or none (a hit is accepted by one comparison and its distance stored by
    # another): no accepted hit moves the bound
    kept = bounded[:, 0] > 0
    assert np.array_equal(bounded[kept, :3].view(np.uint32), first[kept, :3].view(np.uint32)) and kept.sum() > len(rays) // 4
    m = len(rays)
    table = oracle.simple("wpt_oracle_aabb", m * n, 1, np.tile(boxes.view(np.float32), (m, 1)), np.repeat(rays, n, axis=0),
                          out_dtype=np.int32).reshape(m, n) != 0

    plain_visits = folded_visits = to_folded = leaf_tests = 0
    for r in range(m):
        hit = table[r]
        seq_plain, seq_folded = [], []
        node = 0
        while node < n:
            plain_visits += 1
            if hit[node] and kind[node] == INNER:
                node += 1
                to_folded += 1 if same_as_parent[node] and kind[node] == INNER else 0
            else:
                if hit[node] and kind[node] == TRIANGLE:
                    seq_plain.append(int(link[node]))
                node = end[node]
        node = 0
        while node < n:
            folded_visits += 1
            w = int(words[node])
            if hit[node] and w >= 1 << 31:
                seq_folded.append((~w) & 0xffffffff)
                node = end[node]
            else:
                node = w if hit[node] else end[node]
        assert seq_plain == seq_folded, r
        leaf_tests += len(seq_plain)
    print("rays %d: node visits %d unfolded (oracle %d), %d folded, %d to folded children; leaf tests %d (oracle %d); share saved %.4f"
          % (m, plain_visits, counters["node_visits"], folded_visits, to_folded, leaf_tests, counters["leaf_tests"], 1.0 - folded_visits / plain_visits))
    assert plain_visits == counters["node_visits"] and leaf_tests == counters["leaf_tests"]
    assert plain_visits - folded_visits == to_folded
    # The frame's own rays save 14.75 % of their visits by the inner folds (counted with the oracle on the bench scene at 256 x 256,
    # 64 spp).  These rays are another mix -- no light rays, every direction alike, the final bound from the start -- but all
    # of them start inside the room, whose walls' quads are the folded links, so the share is of that size: between half and
    # twice the frame's.
    share = 1.0 - folded_visits / counters["node_visits"]
    assert 0.5 * 0.1475 <= share <= 2.0 * 0.1475, share

