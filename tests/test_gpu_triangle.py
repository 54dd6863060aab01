"""The device's copy of wurblpt_amd/csrc/wpt_triangle.h, case by case: the sets of tests/triangle_rotated.cpp (random, axis ties,
shared edges and vertices, exact zeros, the double-precision fall-back, denormal products, interval ends; 2^18 cases each, with
the select form's result on the host) go through wpt_selftest_triangle in the four forms the kernels call -- rayAux +
triangleTest, rayAuxRotated + triangleTestRotated, and the two forms of the light-pdf loop -- and every word must be the host's:
the accepted flag, a, invDet, U, V, W with the sign of a zero, RayAux::k.  A word that is NaN on the host must be NaN on the
device (which NaN is not compared).  The "exact zeros" set is also held against integer arithmetic over its inputs, and
rayAux / rayAuxRotated and sphereTest against the reference's own vectors in tests/golden/ref_golden.json."""
import numpy as np
import pytest

from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu

N = 1 << 18
FORMS = {0: "rayAux + triangleTest", 1: "rayAuxRotated + triangleTestRotated", 2: "light-pdf loop, select form", 3: "light-pdf loop, rotated form"}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the host data, checked before any GPU work"""
    s = tc.dump(tmp_path_factory.mktemp("triangle_cases"), N)
    tc.check_shares(s)
    return s


@pytest.fixture(scope="module")
def device_words(dev, sets):
    """{(set, form): uint32 [N, 8]}, every launch made once"""
    return {(name, form): dev.selftest_triangle(form, w[:, :17].view(np.float32)) for name, w in sets.items() for form in FORMS}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", tc.SETS)
def test_device_words_are_the_hosts(sets, device_words, name, form):
    host, got = sets[name], device_words[(name, form)]
    want = host[:, tc.ACCEPTED:tc.W + 1]
    have = got[:, 0:6]
    both_nan = tc.is_nan(want) & tc.is_nan(have)
    bad = (want != have) & ~both_nan
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, "%s, %s: %d of %d cases differ (in words %s), the first: case %d, host %s, device %s" % (
        name, FORMS[form], rows.size, len(host), np.nonzero(bad.any(axis=0))[0].tolist(), rows[0],
        ["%08x" % x for x in want[rows[0]]], ["%08x" % x for x in have[rows[0]]])
    k = host[:, tc.K_SELECT if form in (0, 2) else tc.K_ROTATED]
    assert np.array_equal(got[:, 6], k), (name, FORMS[form], "RayAux::k")
    assert not got[:, 7].any()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_exact_zeros_on_the_device_are_the_exact_evaluation(sets, device_words, form):
    got = device_words[("exact zeros", form)]
    tc.assert_exact(sets["exact zeros"], got[:, 0], got[:, 3:6], FORMS[form])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def test_device_ray_helper_is_the_references(dev, golden):
    """RayIntersectionHelper of the reference (inv, kx ky kz, S) against rayAux and, with its swap undone, rayAuxRotated"""
    rays = golden.f32("rayhelper_rays").reshape(-1, 6)
    want = golden.f32("rayhelper_out").reshape(-1, 9)
    assert len(rays) >= 64 and len({tuple(r) for r in want[:, 3:6]}) == 6          # every permutation the helper can choose
    got = dev.selftest_rayaux(rays[:, 3:6])
    assert same_bits(got[:, 0], want), "rayAux"
    assert same_bits(got[:, 1], want), "rayAuxRotated"


def test_device_sphere_test_is_the_references(dev, golden):
    """HitableSphere::hit of the reference, columns haveHit and a, against sphereTest (radius = the largest scaling, as the
    reference's constructor takes it)"""
    rec = golden.f32("sphere_records").reshape(-1, 11)
    rays = golden.f32("sphere_rays").reshape(-1, 8)
    want = golden.f32("sphere_hits").reshape(-1, 14)[:, 0:2]
    assert len(rec) == len(rays) == len(want) >= 1024 and 0.3 < want[:, 0].mean() < 0.95
    spheres = np.concatenate([rec[:, 0:3], rec[:, 8:11].max(axis=1, keepdims=True)], axis=1)
    got = dev.selftest_sphere(spheres, rays)
    assert same_bits(got, want), int((got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=1).sum())
