"""wpt_launch_plan: which passes render a launch -- wavefront form or single kernel, pixel pool or not, and one pass, two
passes, the adaptive order or pixels in slices -- as a pure host function (no device).  The expected plans are written out by
hand from the table of rules in DESIGN.md section 4, "Which passes render a launch"; nothing here restates the rules in code."""
import os
import subprocess

import pytest

from wurblpt_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RGL, ANIM = 256, 512  # feature bits (wpt_device.h)
SENSORS = {"frame": 0, "transient": 1, "views": 2, "adaptive": 3, "tof": 4}
ONE, TWO, ADAPTIVE, SLICED = "one pass", "two passes", "adaptive order", "sliced"
L = 256 * 1024  # lanes a device of 256 compute units holds at once; a launch is pooled from 256 * 256 + 1 pixels on
L8 = 8 * 1024   # ... and one of 8 compute units: pooled from 8 * 256 + 1 pixels on
SLOT_MAX = (1 << 28) - 1


def facts(sensor, block, s, cu=256, lds=0, count=0, need=0, variant=0, wf=0, slices=0):
    return (sensor, block, s, cu, lds, count, need, variant, wf, slices)


# facts -> wavefront, wavefront falls back, pooled, strategy, units, rows, passes
ROWS = [
    # the pixel pool: more workgroups than compute units
    (facts("frame", 256 * 256, 8), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("frame", 256 * 256 + 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 257 * 256, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 8 * 256, 8, cu=8), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("frame", 8 * 256 + 1, 8, cu=8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", (1 << 31) - 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 1 << 31, 8), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 8, variant=0x10), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 8, count=1), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("views", 2 * L, 8, count=1), (0, 0, 0, ONE, 1, 8, 1)),
    # two passes: the scene in HBM, 2 to 64 pixels per lane, 8 rows of strata and more
    (facts("frame", L, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", L + 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L - 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 64 * L, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 64 * L + 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 7), (0, 0, 1, ONE, 1, 7, 1)),
    (facts("frame", 2 * L, 32), (0, 0, 1, TWO, 1, 32, 2)),
    (facts("frame", 2 * L8 - 1, 8, cu=8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L8, 8, cu=8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 64 * L8, 8, cu=8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 64 * L8 + 1, 8, cu=8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 8, variant=0x40), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("frame", 2 * L, 8, need=RGL), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 2 * L, 8, need=ANIM), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("transient", 2 * L, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("tof", 2 * L, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("tof", 2 * L - 1, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("views", 2 * L, 8), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("transient", 2 * L, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("tof", 2 * L, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("views", 2 * L, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    # the adaptive order: any pooled adaptive launch (its samples_sqrt is 1)
    (facts("adaptive", 256 * 256, 1), (0, 0, 0, ONE, 1, 1, 1)),
    (facts("adaptive", 256 * 256 + 1, 1), (0, 0, 1, ADAPTIVE, 1, 1, 1)),
    (facts("adaptive", 2 * L, 1), (0, 0, 1, ADAPTIVE, 1, 1, 1)),
    (facts("adaptive", 2 * L, 1, lds=1), (0, 0, 1, ADAPTIVE, 1, 1, 1)),
    (facts("adaptive", 8 * 256 + 1, 1, cu=8), (0, 0, 1, ADAPTIVE, 1, 1, 1)),
    (facts("adaptive", 2 * L, 1, variant=0x40), (0, 0, 1, ONE, 1, 1, 1)),
    (facts("adaptive", 2 * L, 1, variant=0x10), (0, 0, 0, ONE, 1, 1, 1)),
    # pixels in slices: the frame sensor's kernels with the scene in LDS, more pixels than lanes; the library's own units
    (facts("frame", L, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", L + 1, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L - 1, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 32, lds=1), (0, 0, 1, SLICED, 11, 3, 1)),
    (facts("frame", 4 * L, 32, lds=1), (0, 0, 1, SLICED, 11, 3, 1)),
    (facts("frame", 64 * L, 32, lds=1), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", 64 * L + 1, 32, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 7, lds=1), (0, 0, 1, ONE, 1, 7, 1)),
    (facts("frame", 2 * L, 8, lds=1), (0, 0, 1, SLICED, 4, 2, 1)),
    (facts("frame", 2 * L8, 32, cu=8, lds=1), (0, 0, 1, SLICED, 11, 3, 1)),
    (facts("frame", 2 * L8 - 1, 32, cu=8, lds=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 32, lds=1, variant=0x40), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 32, lds=1, variant=0x10), (0, 0, 0, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 32, lds=1, count=1), (0, 0, 0, ONE, 1, 32, 1)),
    # ... and a forced count: 1 = never, n = 2 .. 15 whatever the pixels per lane, above the lanes at once
    (facts("frame", 2 * L, 32, lds=1, slices=1), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", 2 * L, 32, lds=1, slices=2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", 2 * L, 32, lds=1, slices=15), (0, 0, 1, SLICED, 11, 3, 1)),
    (facts("frame", 2 * L, 32, lds=1, slices=0x100 | 2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", L, 32, lds=1, slices=2), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", L + 1, 32, lds=1, slices=2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", L + 1, 7, lds=1, slices=15), (0, 0, 1, SLICED, 7, 1, 1)),
    (facts("frame", L + 1, 1, lds=1, slices=2), (0, 0, 1, ONE, 1, 1, 1)),
    (facts("frame", 64 * L + 1, 32, lds=1, slices=2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", L8, 32, cu=8, lds=1, slices=2), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", L8 + 1, 32, cu=8, lds=1, slices=2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", 2 * L, 32, slices=2), (0, 0, 1, TWO, 1, 32, 2)),
    # a lane keeps slot | unit << 28 in a register, and the pool's counter must not wrap: units * pixels + 2 * lanes < 2^32
    (facts("frame", SLOT_MAX, 32, lds=1, slices=2), (0, 0, 1, SLICED, 2, 16, 1)),
    (facts("frame", SLOT_MAX + 1, 32, lds=1, slices=2), (0, 0, 1, ONE, 1, 32, 1)),
    (facts("frame", SLOT_MAX, 45, cu=131072, lds=1, slices=15), (0, 0, 1, SLICED, 15, 3, 1)),
    (facts("frame", SLOT_MAX, 45, cu=131073, lds=1, slices=15), (0, 0, 1, ONE, 1, 45, 1)),
    # the wavefront form: one frame without counters of a scene at rest; the library's own choice needs measured BRDFs and 2^21
    # pixels and falls back to the single kernel's plan, a forced one reports its errors
    (facts("frame", (1 << 21) - 1, 8, need=RGL), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 1 << 21, 8, need=RGL), (1, 1, 1, TWO, 1, 8, 2)),
    (facts("frame", (1 << 21) - 1, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 1 << 21, 8), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 1 << 21, 8, need=RGL, cu=8), (1, 1, 1, ONE, 1, 8, 1)),
    (facts("frame", 1 << 21, 8, need=RGL | ANIM), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 1 << 21, 8, need=RGL, count=1), (0, 0, 0, ONE, 1, 8, 1)),
    (facts("frame", 1 << 21, 8, need=RGL, wf=2), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 1 << 21, 8, need=RGL, wf=1), (1, 0, 1, TWO, 1, 8, 2)),
    (facts("frame", 64 * 64, 2, wf=1), (1, 0, 0, ONE, 1, 2, 1)),
    (facts("frame", 64 * 64, 2, wf=2), (0, 0, 0, ONE, 1, 2, 1)),
    (facts("frame", 64 * 64, 2, wf=1, count=1), (0, 0, 0, ONE, 1, 2, 1)),
    (facts("frame", 64 * 64, 2, wf=1, need=ANIM), (0, 0, 0, ONE, 1, 2, 1)),
    (facts("frame", 2 * L, 32, lds=1, wf=1), (1, 0, 1, SLICED, 11, 3, 1)),
    (facts("transient", 1 << 21, 8, need=RGL, wf=1), (0, 0, 1, TWO, 1, 8, 2)),
    (facts("views", 1 << 21, 8, need=RGL, wf=1), (0, 0, 1, ONE, 1, 8, 1)),
    (facts("adaptive", 1 << 21, 1, need=RGL, wf=1), (0, 0, 1, ADAPTIVE, 1, 1, 1)),
    (facts("tof", 1 << 21, 8, need=RGL, wf=1), (0, 0, 1, TWO, 1, 8, 2)),
]


def plan(f):
    sensor, block, s, cu, lds, count, need, variant, wf, slices = f
    p = device.launch_plan(SENSORS[sensor], count, need, lds, block, s, cu, variant, wf, slices)
    return (int(p["wavefront"]), int(p["wavefront_falls_back"]), int(p["pooled"]), p["strategy"], p["units"], p["rows"], p["passes"])


@pytest.mark.parametrize("sensor", sorted(SENSORS))
def test_plan_of_each_row(sensor):
    seen = 0
    for f, expected in ROWS:
        if f[0] == sensor:
            assert plan(f) == expected, f
            seen += 1
    assert seen >= 3


def test_rows_cover_every_switch():
    assert len({f for f, _ in ROWS}) == len(ROWS)
    column = lambda k: {f[k] for f, _ in ROWS}
    assert column(0) == set(SENSORS) and column(3) >= {8, 256} and column(4) == {0, 1} and column(5) == {0, 1}
    assert column(6) == {0, RGL, ANIM, RGL | ANIM} and column(7) == {0, 0x10, 0x40} and column(8) == {0, 1, 2}
    assert column(9) >= {0, 1, 2, 15} and column(2) >= {7, 8}
    assert {e[3] for _, e in ROWS} == {ONE, TWO, ADAPTIVE, SLICED}
    for cu, lanes in ((256, L), (8, L8)):
        blocks = {f[1] for f, _ in ROWS if f[3] == cu}
        assert blocks >= {cu * 256, cu * 256 + 1, 2 * lanes - 1, 2 * lanes, 64 * lanes, 64 * lanes + 1}
    assert {f[1] for f, _ in ROWS} >= {L, L + 1, (1 << 21) - 1, 1 << 21}


def test_the_librarys_own_units_are_those_of_the_slices_plan():
    checked = 0
    for f, expected in ROWS:
        if expected[3] == SLICED and f[9] == 0:
            assert expected[4:6] == device.slices_plan(f[1], f[3] * 1024, f[2]), f
            checked += 1
    assert checked >= 5


def test_a_plan_without_its_facts_is_refused():
    with pytest.raises(RuntimeError, match="sensor"):
        device.launch_plan(5, 0, 0, 0, 1 << 20, 8, 256)
    with pytest.raises(RuntimeError, match="wavefront mode must be 0, 1 or 2"):
        device.launch_plan(0, 0, 0, 0, 1 << 20, 8, 256, 0, 3, 0)


def test_the_plan_on_its_own_under_the_sanitizers(tmp_path):
    """tests/launch_plan_check.cpp: wpt_launch_plan.h compiled outside the library, without a header of HIP or of the kernels, with
    -fsanitize=address,undefined; the plan swept over the cross product of the values around its thresholds keeps its invariants"""
    exe = str(tmp_path / "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-3000:]
    assert " 0 failures" in out and "BROKEN" not in out
    assert not r.stderr, r.stderr.decode()[-2000:]


def test_code_objects_are_recorded_unchanged():
    """profiles/launch_plan_code_objects.txt, written by tools/code_object_compare.sh: every translation unit compiles to the
    same gfx950 code object as before the plan (wpt_capi among them: only its host side changed)"""
    rows = [line.split(" : ") for line in open(os.path.join(ROOT, "profiles", "launch_plan_code_objects.txt")) if not line.startswith("#")]
    verdict = {r[0]: r[-1].strip() for r in rows}
    assert len(verdict) == 46
    assert all(v == "same" for v in verdict.values()), verdict
    assert "wpt_capi" in verdict and "wpt_k_progress" in verdict and sum(u.startswith(("wpt_k_basic", "wpt_k_full")) for u in verdict) == 37
