"""Where a launch in the large form of the rotated kernels keeps the material records that its kernel reads by LDS address
(wurblpt_amd/csrc/wpt_lds_places.h, materialPlaces and launchMaterialPlaces): whole records of eight quadwords, behind the corners
where the kernel choice has them in LDS anyway, else behind the launch's parts of a hit's data as long as they end in front of the
paths' cold words at 32 KiB.  A kernel without parts, and a scene whose records do not fit, read them through the scene's array
like every other kernel.  The functions are pure and are held to rows written out by hand through tests/material_places.cpp, a
program of its own; the same program sweeps random counts against the rules a layout must satisfy and holds hitDataPlaces and
hitDataKernelParts to what they returned before, built with the address and undefined-behaviour sanitizers.

All places are quadwords from the scene's start, 512 bytes into LDS: the room ends at quadword 2016."""
import functools
import os
import subprocess
import tempfile

import pytest

from wurblpt_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "material_places.cpp")
ROOM = (32 * 1024 - 512) // 16
FIELDS = ("fits", "at", "quads", "kernel_parts", "end")


@functools.lru_cache(maxsize=None)
def program(sanitized=False):
    """tests/material_places.cpp, built once per process (and once more with the sanitizers)"""
    exe = os.path.join(tempfile.mkdtemp(prefix="material_places_"), "material_places")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    subprocess.run(["g++"] + flags + ["-Wall", "-Werror", SOURCE, "-o", exe], check=True, timeout=300)
    return exe


def places(nodes, triangles, materials, behind_corners, instances, hotspots):
    out = subprocess.run([program(), "places"] + [str(int(v)) for v in (nodes, triangles, materials, behind_corners, instances, hotspots)],
                         capture_output=True, check=True, timeout=60).stdout.split()
    return dict(zip(FIELDS, (int(v) for v in out)))


# the Cornell box (71 nodes, 36 triangles, 2 hot spots, 6 materials, no transformed triangle): records and hot spots end at 1772
# (tests/test_hit_data_layout.py), the six material records of 8 quadwords follow and end at 1820
ROWS = [
    ("the Cornell box", (71, 36, 6, False, 0, 2), dict(fits=1, at=1772, quads=1820, kernel_parts=3, end=1772)),
    ("the Cornell box, transformed instances", (71, 36, 6, False, 18, 2), dict(fits=1, at=1826, quads=1874, kernel_parts=7, end=1826)),
    # in LDS behind the corners anyway (144 node quadwords, 324 of corners): read there, nothing is added behind the parts
    ("the Cornell box, materials behind the corners", (71, 36, 6, True, 18, 2), dict(fits=1, at=468, quads=1874, kernel_parts=7, end=1874)),
    # either side of the cold words: 2016 - 1772 = 244 quadwords are 30 records and a half
    ("the last count that fits", (71, 36, 30, False, 0, 2), dict(fits=1, at=1772, quads=2012, kernel_parts=3, end=1772)),
    ("the first that does not", (71, 36, 31, False, 0, 2), dict(fits=0, at=1772, quads=1772, kernel_parts=3, end=1772)),
    # ... and to the quadword: four normal matrices end at 1784, 29 records at 2016, the room's last quadword
    ("ends with the room's last byte", (71, 36, 29, False, 4, 2), dict(fits=1, at=1784, quads=2016, kernel_parts=7, end=1784)),
    ("ends one record behind it", (71, 36, 30, False, 4, 2), dict(fits=0, at=1784, quads=1784, kernel_parts=7, end=1784)),
    ("no materials", (71, 36, 0, False, 0, 2), dict(fits=0, at=1772, quads=1772, kernel_parts=3, end=1772)),
    # a kernel without parts (no hot spot; node copies that leave no room) reads the records like every other kernel
    ("no hot spot: a kernel without parts", (71, 36, 6, False, 0, 0), dict(fits=0, at=1504, quads=1504, kernel_parts=0, end=1756)),
    ("nothing fits behind the node copies", (101, 36, 6, False, 18, 2), dict(fits=0, at=2000, quads=2000, kernel_parts=0, end=2000)),
    # far beyond the room: nothing overflows
    ("2^32 - 1 materials", (71, 36, 0xffffffff, False, 0, 2), dict(fits=0, at=1772, quads=1772, kernel_parts=3, end=1772)),
    ("2^29 materials (2^32 quadwords)", (71, 36, 1 << 29, False, 0, 2), dict(fits=0, at=1772, quads=1772, kernel_parts=3, end=1772)),
    ("2^32 - 1 of everything", (0xffffffff,) * 3 + (True,) + (0xffffffff,) * 2, dict(fits=0, at=0xffffffff, quads=0xffffffff, kernel_parts=0, end=0xffffffff)),
]


@pytest.mark.parametrize("name,counts,expected", ROWS, ids=[r[0] for r in ROWS])
def test_rows_written_out_by_hand(name, counts, expected):
    got = places(*counts)
    assert got == expected, (name, got)


@pytest.mark.parametrize("name,counts,expected", ROWS, ids=[r[0] for r in ROWS])
def test_records_lie_in_front_of_the_cold_words_and_overlap_nothing(name, counts, expected):
    nodes, triangles, materials, behind, instances, hotspots = counts
    p = places(*counts)
    if not p["fits"]:
        return
    start, end = p["at"], p["at"] + 8 * materials
    assert end <= ROOM and p["quads"] <= ROOM
    node_quads, corners = 2 * nodes + 2, 9 * triangles
    assert start >= node_quads + corners                     # behind copy 0 of the nodes and the corners
    if behind:
        # ... and in front of copies 1 .. 7 of the nodes, which lie behind everything that follows copy 0
        stride = ((node_quads + 13) & ~15) + 2
        used = node_quads + corners + 8 * materials
        base = ((used - stride + 15) & ~15) if used > stride else 0
        assert end <= base + stride
    else:
        assert start == p["end"] and p["quads"] == end       # behind the parts of a hit's data, and the whole ends with them


def test_the_bench_scene_has_the_counts_of_the_first_row():
    d = host.cornell(64, 64, 1, 2).d
    assert (d.node_count, d.tri_count, d.material_count, d.hotspot_count) == (71, 36, 6, 2)


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
