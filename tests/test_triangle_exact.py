"""The sets of tests/triangle_rotated.cpp as the device tests use them, checked here on the CPU (tests/triangle_cases.py): the
program's `--dump` mode writes cases and the select form's host result; the sets must have the shares that make the device
comparison mean something (no NaN outside the denormal set and at most 10 % there, the fall-back set in the fall-back, denormal
U, V, W in the denormal set, both outcomes at the interval's ends), and the "exact zeros" set -- small integers, every value
exact in any precision -- must come out as integer and rational arithmetic over its inputs says."""
import numpy as np
import pytest

from tests import triangle_cases as tc

N = 1 << 18


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return tc.dump(tmp_path_factory.mktemp("triangle_cases"), N)


def test_the_sets_have_the_shares_the_device_tests_rely_on(sets):
    s = tc.check_shares(sets)
    for name in tc.SETS:
        print("%-28s accepted %.4f fall-back %.4f NaN word %.4f non-finite word %.4f denormal U, V or W among accepted %.4f" % (
            name, s[name]["accepted"], s[name]["fallback"], s[name]["nan"], s[name]["nonfinite"], s[name]["denormal"]))
    assert s["denormal products"]["nonfinite"] > 0.01    # the infinite invDet (1 / a denormal det) is there to be compared
    assert s["exact zeros"]["fallback"] > 0.1 and s["shared edges and vertices"]["fallback"] > 0.1
    # every rotation and both signs of the largest component, in every set (RayAux::k of the rotated form)
    for name, w in sets.items():
        kz = (w[:, tc.K_ROTATED] >> 4) & 3
        assert min((kz == k).mean() for k in range(3)) > 0.1, name
        assert 0.25 < ((w[:, tc.K_ROTATED] & tc.RAY_FLIP) != 0).mean() < 0.75, name


def test_a_dump_does_not_depend_on_the_number_of_threads(sets, tmp_path, monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    again = tc.dump(tmp_path, 4096)
    for name in tc.SETS:
        assert np.array_equal(again[name], sets[name][:4096]), name


def test_exact_zeros_host_result_is_the_exact_evaluation(sets):
    w = sets["exact zeros"]
    tc.assert_exact(w, w[:, tc.ACCEPTED], w[:, tc.U:tc.W + 1], "host")


def test_integer_and_rational_evaluation_agree(sets):
    w = sets["exact zeros"][:3000]
    accepted, uvw = tc.exact_set(w)
    f = w[:, :17].view(np.float32)
    for i in range(len(w)):
        a, u, v, x = tc.exact_case(f[i])
        assert a == accepted[i] and (float(u), float(v), float(x)) == tuple(uvw[i]), i


def test_the_exact_check_notices_a_wrong_result(sets):
    """the comparison is not vacuous: a flipped flag and a U off by one unit in the last place are both found"""
    w = sets["exact zeros"]
    flags = w[:, tc.ACCEPTED].copy()
    flags[np.nonzero(flags == 0)[0][0]] = 1
    with pytest.raises(AssertionError):
        tc.assert_exact(w, flags, w[:, tc.U:tc.W + 1], "flag")
    uvw = w[:, tc.U:tc.W + 1].copy()
    row = np.nonzero((w[:, tc.ACCEPTED] == 1) & (uvw[:, 0] != 0))[0][0]
    uvw[row, 0] += 1
    with pytest.raises(AssertionError):
        tc.assert_exact(w, w[:, tc.ACCEPTED], uvw, "ulp")
