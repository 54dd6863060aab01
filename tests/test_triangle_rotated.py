"""wurblpt_amd/csrc/wpt_triangle.h on the CPU: triangleTestRotated -- the watertight test on corners and origin stored in the order
of the ray's largest direction component, the reference's swap of kx and ky as a flip of sign bits -- against triangleTest, on the
bits of accepted, a, invDet, U, V, W: 10^8 random rays and triangles and six adversarial sets (the kz ties of rayAux, rays through
shared edges and vertices, integer cases whose U, V, W are exactly zero with either sign, the double-precision fall-back, products
in the denormal range, and accepted cases again with an end of the interval at their own a or next to it).  The program (tests/triangle_rotated.cpp) prints cases and differences per set; every set must be there, filled, and without a difference."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINE = re.compile(r"^(.+): (\d+) cases, (\d+) accepted, (\d+) fall-back, (\d+) swapped, kz (\d+) (\d+) (\d+), (\d+) differences$")


def test_rotated_triangle_test_equals_the_select_form_bit_for_bit(tmp_path):
    exe = str(tmp_path / "triangle_rotated")
    subprocess.run(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "triangle_rotated.cpp"), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, "100000000"], capture_output=True, timeout=1500)
    out = r.stdout.decode()
    print(out)
    sets = {}
    for line in out.splitlines():
        m = LINE.match(line)
        if m:
            sets[m.group(1)] = [int(x) for x in m.groups()[1:]]
    assert set(sets) == {"random", "axis ties", "shared edges and vertices", "exact zeros", "double-precision fall-back", "denormal products",
                         "interval ends"}, out
    for name, (cases, accepted, fallback, swapped, kz0, kz1, kz2, differences) in sets.items():
        assert cases >= (100000000 if name == "random" else 1000000), (name, cases)
        assert accepted > cases // 10000, (name, accepted)            # hits are compared value by value: there must be some
        assert cases // 4 < swapped < cases - cases // 4, (name, swapped)  # both signs of the largest component
        assert min(kz0, kz1, kz2) > cases // 10, (name, kz0, kz1, kz2)  # every rotation
        assert differences == 0, (name, differences)
    assert sets["double-precision fall-back"][2] > sets["double-precision fall-back"][0] // 2   # the set does enter the fall-back
    assert sets["denormal products"][2] == sets["denormal products"][0]                             # every one of them
    assert sets["interval ends"][0] // 4 < sets["interval ends"][1] < sets["interval ends"][0] - sets["interval ends"][0] // 4   # both outcomes
    assert sets["exact zeros"][2] > 100000 and sets["shared edges and vertices"][2] > 100000     # U, V or W zero or nearly so
    assert r.returncode == 0 and "total: 0 differences" in out, out
