"""wpt_slices_plan, the library's own choice of how a pooled launch cuts its pixels into units of strata rows: a pure host
function (no device)."""
from wurblpt_amd import device


def test_plan_over_a_grid():
    sliced = 0
    for lanes in (1024, 65536, 262144, 311296):
        for per_lane in (0.5, 1.0, 1.99, 2.0, 2.5, 4.0, 16.0, 64.0, 64.01, 200.0):
            block = int(lanes * per_lane)
            for s in list(range(1, 40)) + [63, 64, 100, 255, 1000, 1024, 4096, 65535]:
                units, rows = device.slices_plan(block, lanes, s)
                assert 1 <= units <= 15, (block, lanes, s, units, rows)
                assert rows >= 1
                assert (units - 1) * rows < s <= units * rows, (block, lanes, s, units, rows)
                if block < 2 * lanes or block > 64 * lanes or s < 8:
                    assert units == 1, (block, lanes, s, units)
                elif units > 1:
                    assert rows >= 2, (block, lanes, s, units, rows)
                    sliced += 1
    assert sliced > 0


def test_plan_of_the_measured_frames():
    """the Cornell frames of tools/slice_rate.py on 256 compute units: 11 units for the bench frame, 2 at 16 pixels per lane,
    none at 64 (where a unit's start costs more than the end of the launch is worth)"""
    lanes = 256 * 1024
    assert device.slices_plan(1024 * 1024, lanes, 32) == (11, 3)
    assert device.slices_plan(2048 * 2048, lanes, 16) == (2, 8)
    assert device.slices_plan(4096 * 4096, lanes, 8) == (1, 8)
    assert device.slices_plan(1024 * 640, lanes, 8) == (3, 3)


def test_plan_without_lanes_is_unsliced():
    assert device.slices_plan(1 << 20, 0, 32) == (1, 32)


def test_code_objects_of_the_existing_units_are_recorded_unchanged():
    """profiles/sliced_code_objects.txt, written by tools/code_object_compare.sh: every translation unit the parent commit had
    compiles to the same gfx950 code object from this tree's sources, and the two sliced twins are new"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [line.split(" : ") for line in open(os.path.join(root, "profiles", "sliced_code_objects.txt")) if not line.startswith("#")]
    verdict = {r[0]: r[-1].strip() for r in rows}
    new = sorted(u for u, v in verdict.items() if v == "new")
    assert new == ["wpt_k_basic_lds_rot_sliced", "wpt_k_basic_lds_sliced"]
    assert all(v == "same" for u, v in verdict.items() if u not in new), verdict
    assert len(verdict) == 45
