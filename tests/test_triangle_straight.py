"""wurblpt_amd/csrc/wpt_triangle.h on the CPU: triangleTestRotatedStraight -- the leaf pass of the kernels with the scene in LDS,
the watertight test in one straight run with its three rejections combined at the end -- against triangleTestRotated, which
returns at the first rejection.  Both run over the seven sets of tests/triangle_rotated.cpp (2^18 cases each) and over one more
set made in tests/triangle_straight.cpp: ordinary cases mixed with corners on the ray (det == 0, 1 / det infinite, a NaN),
zero-area triangles, NaN corners (accepted, as in the reference), infinite invDet, and amin or amax at the case's own a.  The
accepted flag must be equal for every case and, where accepted, the bits of a, invDet, U, V, W, signs of zeros included (which
NaN is not compared); the branching form's result must also be the one the dump carries from the select form."""
import pytest

from tests import triangle_cases as tc
from tests import triangle_straight_cases as sc

N = 1 << 18


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    sets, report, kinds, out = sc.run(tmp_path_factory.mktemp("triangle_straight"), N)
    print(out)
    return sets, report, kinds, out


@pytest.mark.parametrize("name", sc.SETS)
def test_straight_form_equals_the_branching_form_bit_for_bit(result, name):
    _, report, _, out = result
    assert set(report) == set(sc.SETS), out
    cases, accepted, straight_alone, branching_alone, words, not_the_files = report[name]
    assert cases == N and accepted > N // 10000, (name, cases, accepted)   # hits are compared word by word: there must be some
    assert (straight_alone, branching_alone, words, not_the_files) == (0, 0, 0, 0), (name, report[name])


def test_the_extra_set_holds_what_the_straight_form_alone_computes(result):
    sets, report, kinds, out = result
    assert kinds is not None and "total: 0 differences" in out, out
    cases, accepted = dict(zip(sc.KINDS, kinds["cases"])), dict(zip(sc.KINDS, kinds["accepted"]))
    assert min(cases.values()) >= N // 7 and sum(cases.values()) == N
    assert 0.1 < accepted["ordinary"] / cases["ordinary"] < 0.9                        # ordinary hits and misses beside the rest
    assert accepted["corners on the ray"] == 0 and accepted["zero-area triangle"] == 0   # det == 0 or mixed signs
    assert accepted["NaN corner"] == cases["NaN corner"]                               # every comparison false: accepted
    assert accepted["infinite invDet"] > cases["infinite invDet"] // 2
    for end in ("amin at a", "amax at a"):                                             # both outcomes at either end
        assert 0.2 < accepted[end] / cases[end] < 0.8, (end, accepted[end])
    assert kinds["zero_det"] >= cases["corners on the ray"]                            # the straight form did divide by zero there
    assert kinds["infinite_inv_det"] >= cases["corners on the ray"] + cases["infinite invDet"] // 2
    assert kinds["nan"] >= cases["corners on the ray"] + cases["NaN corner"]
    w = sets[sc.EXTRAS]
    assert int((w[:, tc.ACCEPTED] == 1).sum()) == report[sc.EXTRAS][1]                # the file is the run's
    assert tc.is_nan(w[:, tc.A:tc.W + 1]).any(axis=1).sum() >= cases["NaN corner"]
