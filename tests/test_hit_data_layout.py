"""Where the large form of the rotated kernels keeps a hit's data in LDS (wurblpt_amd/csrc/wpt_lds_places.h, hitDataPlaces): a
record of seven quadwords per triangle, eight per hot spot and three per instance's normal matrix, in that order behind the node
copies, as long as they end in front of the paths' cold words at 32 KiB.  The function is pure and is held to rows written out
by hand through tests/hit_data_layout.cpp, a program of its own; the same program sweeps a few thousand random counts against
the rules a layout must satisfy, built with the address and undefined-behaviour sanitizers.  The parts are template arguments of
the kernels, which exist for all three parts, for records and hot spots, and for none (hitDataKernelParts).

All places are quadwords from the scene's start, 512 bytes into LDS: the room ends at quadword 2016.  A place is a whole number
of quadwords, so the rows either side of the cold words are the scene that ends exactly there and the next larger one."""
import functools
import os
import subprocess
import tempfile

import pytest

from wurblpt_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "hit_data_layout.cpp")
RECORDS, HOTSPOTS, NORMALS = 1, 2, 4
ROOM = (32 * 1024 - 512) // 16      # 2016 quadwords between the math tables and the cold words
FIELDS = ("parts", "records_at", "hotspots_at", "normals_at", "node_copies_end", "quads", "kernel_parts")


@functools.lru_cache(maxsize=None)
def program(sanitized=False):
    """tests/hit_data_layout.cpp, built once per process (and once more with the sanitizers)"""
    exe = os.path.join(tempfile.mkdtemp(prefix="hit_data_layout_"), "hit_data_layout")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    subprocess.run(["g++"] + flags + ["-Wall", "-Werror", SOURCE, "-o", exe], check=True, timeout=300)
    return exe


def places(nodes, triangles, materials, instances, hotspots):
    """hitDataPlaces for these counts as a dict of FIELDS (materials: the records in LDS; instances: those a transformed
    triangle names)"""
    out = subprocess.run([program(), "places"] + [str(v) for v in (nodes, triangles, materials, instances, hotspots)], capture_output=True,
                         check=True, timeout=60).stdout.split()
    return dict(zip(FIELDS, (int(v) for v in out)))


# the Cornell box: 71 nodes and 36 triangles.  A node copy is 2 * 71 + 2 = 144 quadwords, the corners 3 * 108 = 324, the material
# records stay in HBM; the copies' stride is 144 + 2, copy 1 .. 7 lie at 336 + 146 k (336: 468 - 146 = 322 rounded up to 16), so
# the node copies end at 336 + 8 * 146 = 1504.  36 records of 7 end at 1756, 2 hot spots of 8 at 1772.
CORNELL = dict(parts=RECORDS | HOTSPOTS, records_at=1504, hotspots_at=1756, normals_at=1772, node_copies_end=1504, quads=1772)
ROWS = [
    # the bench scene: no triangle of it is transformed, so no normal matrix is asked for
    ("the Cornell box", (71, 36, 0, 0, 2), CORNELL),
    # ... and with its boxes as transformed instances: 18 matrices of 3
    ("the Cornell box, transformed instances", (71, 36, 0, 18, 2), dict(CORNELL, parts=7, quads=1772 + 54)),
    # with its six material records in LDS (48 quadwords): 516 used, copies at 384 + 146 k, all of it 48 later
    ("the Cornell box, materials in LDS", (71, 36, 6, 18, 2),
     dict(parts=7, records_at=1552, hotspots_at=1804, normals_at=1820, node_copies_end=1552, quads=1874)),
    # records and hot spots fit, the normal matrices do not: 1772 + 3 * 82 = 2018
    ("records in, normal matrices out", (71, 36, 0, 82, 2), CORNELL),
    ("one matrix fewer: all in", (71, 36, 0, 81, 2), dict(CORNELL, parts=7, quads=2015)),
    # either side of the cold words: 31 hot spots end at 1756 + 248 = 2004, 4 matrices at 2016, the room's last quadword; 5 at 2019
    ("ends with the room's last byte", (71, 36, 0, 4, 31), dict(CORNELL, parts=7, normals_at=2004, quads=2016)),
    ("ends behind it", (71, 36, 0, 5, 31), dict(CORNELL, normals_at=2004, quads=2004)),
    ("hot spots end behind it: what follows stays out too", (71, 36, 0, 1, 33), dict(CORNELL, parts=RECORDS, normals_at=1756, quads=1756)),
    # a part with nothing to hold is not in, and the next one is asked
    ("no hot spots", (71, 36, 0, 18, 0), dict(CORNELL, parts=RECORDS | NORMALS, normals_at=1756, quads=1756 + 54)),
    ("no transformed instance", (71, 36, 0, 0, 2), CORNELL),
    ("neither", (71, 36, 0, 0, 0), dict(CORNELL, parts=RECORDS, normals_at=1756, quads=1756)),
    # the node copies nearly fill the room: 101 nodes are 204 quadwords, stride 210, the scene in front 204 + 324 = 528, so the
    # copies lie at 320 + 210 k and end at 2000.  The 16 quadwords left would hold the two hot spots, but the records come first
    ("nothing fits", (101, 36, 0, 18, 2), dict(parts=0, records_at=2000, hotspots_at=2000, normals_at=2000, node_copies_end=2000, quads=2000)),
    # more instances than the launch's word can name
    # (3 nodes: copies of 8 quadwords at 18 k, the triangle's corners behind copy 0)
    ("65 536 instances", (3, 1, 0, 65536, 1), dict(parts=RECORDS | HOTSPOTS, records_at=144, hotspots_at=151, normals_at=159, node_copies_end=144, quads=159)),
]


@pytest.mark.parametrize("name,counts,expected", ROWS, ids=[r[0] for r in ROWS])
def test_rows_written_out_by_hand(name, counts, expected):
    got = places(*counts)
    # the kernels exist for three sets of parts: a launch runs the largest of all three, records and hot spots, none that fits
    kernel = got.pop("kernel_parts")
    assert got == expected, (name, got)
    assert kernel == (7 if expected["parts"] == 7 else 3 if expected["parts"] & 3 == 3 else 0)


def ranges(nodes, triangles, materials, p):
    """[from, to) in quadwords of everything the scene keeps in LDS: copy 0 of the nodes, corners, materials, copies 1 .. 7, and
    the parts that are in; then the cold words"""
    node_quads, corners, mats = 2 * nodes + 2, 9 * triangles, 8 * materials
    stride = ((node_quads + 13) & ~15) + 2
    used = node_quads + corners + mats
    base = ((used - stride + 15) & ~15) if used > stride else 0
    r = [("nodes", 0, node_quads), ("corners", node_quads, node_quads + corners), ("materials", node_quads + corners, used)]
    r += [("node copy %d" % k, base + k * stride, base + k * stride + node_quads) for k in range(1, 8)]
    return r


@pytest.mark.parametrize("name,counts,expected", ROWS, ids=[r[0] for r in ROWS])
def test_parts_overlap_nothing(name, counts, expected):
    """the parts that are in lie behind the node copies, the corners and the materials, one behind the other, and end in front of
    the cold words"""
    nodes, triangles, materials, instances, hotspots = counts
    p = places(*counts)
    fixed = ranges(nodes, triangles, materials, p)
    assert max(to for _, _, to in fixed) <= p["node_copies_end"]      # (a copy's stride is at least 2 more than a copy)
    parts = [(bit, at, at + size) for bit, at, size in ((RECORDS, p["records_at"], 7 * triangles), (HOTSPOTS, p["hotspots_at"], 8 * hotspots),
                                                        (NORMALS, p["normals_at"], 3 * instances)) if p["parts"] & bit]
    for bit, start, end in parts:
        assert start < end <= ROOM, (name, bit)
        for what, a, b in fixed:
            assert end <= a or b <= start or a == b, (name, bit, what)
    for (_, _, end), (_, start, _) in zip(parts, parts[1:]):
        assert end == start
    assert p["quads"] == (parts[-1][2] if parts else p["node_copies_end"]) and (not parts or p["quads"] <= ROOM)


def test_the_bench_scene_has_the_counts_of_the_first_row():
    d = host.cornell(64, 64, 1, 2).d
    assert (d.node_count, d.tri_count, d.hotspot_count) == (71, 36, 2)
    assert not any(d.tri_geom[i].flags & 4 for i in range(d.tri_count))     # WPT_TRI_TRANSFORM


def sweep(exe, cases):
    r = subprocess.run([exe, "sweep", str(cases)], capture_output=True, timeout=600)
    out = r.stdout.decode() + r.stderr.decode()
    print(out)
    assert r.returncode == 0, out
    assert "cases %d, violations 0" % cases in out and "cases covered: yes" in out, out


def test_random_counts_keep_the_rules():
    sweep(program(), 200000)


def test_random_counts_under_the_host_sanitizers():
    sweep(program(sanitized=True), 5000)
