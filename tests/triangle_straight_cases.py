"""tests/triangle_straight.cpp as data -- shared by tests/test_triangle_straight.py (CPU) and tests/test_gpu_leaf_straight.py
(device): the seven sets of tests/triangle_rotated.cpp (tests/triangle_cases.py) go through the program, which compares
triangleTestRotated with triangleTestRotatedStraight case by case and makes one more set, "straight extras"."""
import os
import re
import subprocess

import numpy as np

from tests import triangle_cases as tc

ROOT = tc.ROOT
EXTRAS = "straight extras"
SETS = tc.SETS + [EXTRAS]
KINDS = ["ordinary", "corners on the ray", "zero-area triangle", "NaN corner", "infinite invDet", "amin at a", "amax at a"]
LINE = re.compile(r"^(.+): (\d+) cases, (\d+) accepted, (\d+) straight alone, (\d+) branching alone, (\d+) words differ, (\d+) not the file's$")
KIND_LINE = re.compile(r"^straight extras kinds: ((?:\d+ ){6}\d+), accepted ((?:\d+ ){6}\d+), det == 0 (\d+), infinite invDet (\d+), NaN (\d+)$")


def run(directory, cases_per_set):
    """compiles and runs the program over the dump of tests/triangle_rotated.cpp.  Returns (sets, report, kinds, output):
    sets {name: uint32 [cases_per_set, 26]} with the extras; report {name: [cases, accepted, straight alone, branching alone,
    words, not the file's]}; kinds {"cases": [7], "accepted": [7], "zero_det", "infinite_inv_det", "nan"} of the extras"""
    directory = str(directory)
    sets = dict(tc.dump(directory, cases_per_set))
    exe, cases, extra = (os.path.join(directory, n) for n in ("triangle_straight", "straight_cases.bin", "straight_extra.bin"))
    np.concatenate([sets[name] for name in tc.SETS]).tofile(cases)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "triangle_straight.cpp"), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe, cases, extra, str(cases_per_set)], capture_output=True, timeout=600)
    out = r.stdout.decode()
    assert r.returncode in (0, 1), out + r.stderr.decode()
    sets[EXTRAS] = np.fromfile(extra, dtype=np.uint32).reshape(cases_per_set, tc.WORDS)
    os.remove(cases)
    os.remove(extra)
    report, kinds = {}, None
    for line in out.splitlines():
        m = LINE.match(line)
        if m:
            report[m.group(1)] = [int(x) for x in m.groups()[1:]]
        m = KIND_LINE.match(line)
        if m:
            kinds = {"cases": [int(x) for x in m.group(1).split()], "accepted": [int(x) for x in m.group(2).split()],
                     "zero_det": int(m.group(3)), "infinite_inv_det": int(m.group(4)), "nan": int(m.group(5))}
    return sets, report, kinds, out
