"""wptm::sincosf_ (wurblpt_amd/csrc/wpt_math.h) evaluates the sine and the cosine of one angle with one reduction and without a
branch.  tests/sincos_fused.cpp compares it with wptm::sinf_ and wptm::cosf_ -- which tests/test_math_exact.py pins to the C library
and which the oracle evaluates -- on every one of the 2^32 float bit patterns: 0 differences, no tolerance, no sampling.  The
header's other form (WPT_SINCOSF_POLY_BRANCH: shared reduction, each polynomial behind its branch), which some translation units
keep for their registers, is checked in the same way."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("define", [None, "-DWPT_SINCOSF_POLY_BRANCH"])
def test_sincos_pair_equals_sine_and_cosine_for_every_float(tmp_path, define):
    exe = str(tmp_path / "sincos_fused")
    # fma_d is the IEEE fused multiply-add with or without the instruction: a CPU without it takes the C library's, slower
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
    cmd = ["g++", "-O2"] + fma + ["-ffp-contract=off", "-fopenmp"] + ([define] if define else [])
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "sincos_fused.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, timeout=1500)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert "sine of sincosf_ all 2^32 arguments: 0 differences" in out, out
    assert "cosine of sincosf_ all 2^32 arguments: 0 differences" in out, out
    assert "total: 0 differences" in out, out
