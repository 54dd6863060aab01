"""wurblpt_amd/csrc/wpt_camera_origin.h on the CPU: cameraOriginAtRest -- the origin of a camera's rays, which the large form of the
kernels with the scene in LDS evaluates once per launch and keeps in its launch record -- against the expression blockNewFrom
evaluates per sample (tests/camera_origin.cpp has it written out), compiled with -ffp-contract=off like the kernels.  The three
words must be equal bit for bit (a NaN counts as equal to a NaN) over random poses and over the adversarial set: zero and
negative-zero translation components; negative, zero, negative-zero, denormal, infinite and NaN scaling; non-unit quaternions.
The same program is built once more with the address and undefined-behaviour sanitizers and run as it is."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "camera_origin.cpp")
N = 1 << 17
ADVERSARIAL = 6 * 64 * 512   # quaternions x translations x scalings
LINE = re.compile(r"^(\w+): (\d+) cases, (\d+) words differ, (\d+) from the unfolded evaluation, (\d+) not the translation$")


@functools.lru_cache(maxsize=None)
def report(sanitized):
    exe = os.path.join(tempfile.mkdtemp(prefix="camera_origin_"), "camera_origin")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    subprocess.run(["g++"] + flags + ["-ffp-contract=off", "-Wall", "-Wextra", "-Werror", SOURCE, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(N)], capture_output=True, timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode in (0, 1), out + r.stderr.decode()
    sets = {m.group(1): [int(x) for x in m.groups()[1:]] for m in map(LINE.match, out.splitlines()) if m}
    return sets, out, r.returncode


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "address and undefined-behaviour sanitizers"])
def test_the_function_is_the_blocks_expression_bit_for_bit(sanitized):
    sets, out, status = report(sanitized)
    assert set(sets) == {"random", "adversarial"}, out
    assert sets["random"][0] == N and sets["adversarial"][0] == ADVERSARIAL, out
    for name, (cases, words, unfolded, _) in sets.items():
        assert (words, unfolded) == (0, 0), (name, out)
    assert status == 0 and "total: 0 differences" in out, out


def test_the_origin_is_not_always_the_translation():
    """why nothing of the expression is folded: 0 * s is -0 for a negative s and NaN for an infinite or NaN one, and what the
    rotation makes of that is added to the translation.  A zero translation component so turns -0 or NaN in most of the
    adversarial poses; the random ones (finite scaling, translations away from zero) give the translation itself"""
    sets, out, _ = report(False)
    assert sets["adversarial"][3] > ADVERSARIAL // 2, out
    assert sets["random"][3] == 0, out
