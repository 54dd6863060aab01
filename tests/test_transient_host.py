"""The transient film (SensorRGBTransient, wpt_render_transient_block*) without a GPU: the public headers build, the uniform
edges of the C++ class and of the Python helper are the same floats, bad edge sets are refused before a device is needed,
and the entry points are exported."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
INVALID_ARGUMENT = 1

EDGES_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <wurblpt/wurblpt.hpp>
using namespace WurblPT;
int main(int argc, char* argv[])
{
    if (argc == 2) { /* explicit edges, comma separated: prints "refused" or the bin count */
        std::vector<float> e;
        for (char* t = strtok(argv[1], ","); t; t = strtok(nullptr, ","))
            e.push_back(strtof(t, nullptr));
        try {
            SensorRGBTransient s(4, 3, e);
            printf("%u\n", s.binCount());
        } catch (const std::invalid_argument&) {
            printf("refused\n");
        }
        return 0;
    }
    SensorRGBTransient s(4, 3, strtof(argv[1], nullptr), strtof(argv[2], nullptr), unsigned(atoi(argv[3])));
    for (float e : s.binEdges()) {
        unsigned int bits;
        memcpy(&bits, &e, 4);
        printf("%08x\n", bits);
    }
    printf("%u %zu %zu\n", s.binCount(), s.bin(s.binCount() - 1).dimension(0), s.bin(0).dimension(1));
    return 0;
}
"""


def compile_cpp(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe, *extra]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def test_light_in_flight_example_builds_and_needs_a_device(tmp_path):
    import torch
    exe = compile_cpp(tmp_path, os.path.join(ROOT, "examples", "light_in_flight.cpp"), "light_in_flight")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the run is covered by tests/test_gpu_transient.py")
    r = subprocess.run([exe, "16", "12", "1", "4", "2", "0.5", str(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"no HIP device" in r.stderr
    assert not os.path.exists(str(tmp_path / "frame.pfm"))       # nothing is faked on the CPU


@pytest.mark.parametrize("start,width,count", [(0.0, 1.5, 8), (2.0, 0.125, 64), (0.1, 0.3, 256), (3.3, 0.07, 100), (-1.0, 1e-3, 17)])
def test_uniform_edges_of_the_sensor_and_of_python_are_the_same_floats(tmp_path, start, width, count):
    src = tmp_path / "edges.cpp"
    src.write_text(EDGES_PROGRAM)
    exe = compile_cpp(tmp_path, str(src), "edges")
    out = subprocess.run([exe, repr(start), repr(width), str(count)], capture_output=True, check=True, timeout=60).stdout.decode().split()
    cpp = np.array([int(x, 16) for x in out[:count + 1]], np.uint32)
    assert out[count + 1:] == [str(count), "4", "3"]
    py = device.uniform_edges(start, width, count)
    assert py.dtype == np.float32 and py.shape == (count + 1,)
    assert np.array_equal(cpp, py.view(np.uint32))
    # two roundings: the product, then the sum (a fused multiply-add would round once)
    k = np.arange(count + 1, dtype=np.float32)
    assert np.array_equal(py, np.float32(start) + (k * np.float32(width)).astype(np.float32))


def test_sensor_and_helper_refuse_edges_that_do_not_increase(tmp_path):
    src = tmp_path / "edges.cpp"
    src.write_text(EDGES_PROGRAM)
    exe = compile_cpp(tmp_path, str(src), "edges")
    run = lambda arg: subprocess.run([exe, arg], capture_output=True, check=True, timeout=60).stdout.decode().strip()
    assert run("0,1,2,inf") == "3"
    for bad in ("0,1,1,2", "0,2,1", "0,inf,5", "-inf,0,1", "0,nan,1", "5"):
        assert run(bad) == "refused", bad
    with pytest.raises(ValueError):
        device.uniform_edges(1e8, 1.0, 4)          # 1e8 + 1 rounds to 1e8
    with pytest.raises(ValueError):
        device.uniform_edges(0.0, 0.0, 4)


def _transient_device(edges, count, scene=None, frame=None, bins=None):
    L = device.lib()
    arr = None if edges is None else np.ascontiguousarray(edges, dtype=np.float32)
    ptr = None if arr is None else C.c_void_p(arr.ctypes.data)
    st = L.wpt_render_transient_block_device(scene, None, None, ptr, count, 16, 16, 1, 0, 256, frame, bins, None)
    return st, L.wpt_last_error().decode()


def test_bad_edge_sets_are_refused_without_a_device():
    inf, nan = np.inf, np.nan
    bad = [(None, 4, "NULL"), ([0, 1], 0, "bin count"), ([0.0] * (4098), 4097, "bin count"), ([0, nan, 2], 2, "NaN"),
           ([0, 2, 2, 3], 3, "increase"), ([0, 3, 2], 2, "increase"), ([0, inf, inf], 2, "infinite"), ([-inf, 0, 1], 2, "infinite"),
           ([0, 1, -inf], 2, "infinite"), ([0, 1, 2, inf, 5], 4, "infinite")]
    for edges, count, what in bad:
        st, msg = _transient_device(edges, count, frame=C.c_void_p(16), bins=C.c_void_p(16))
        assert st == INVALID_ARGUMENT and "transient film" in msg and what in msg, (edges, count, msg)
    # a good set passes the edge check: what is refused then is the missing scene
    for edges in ([0, 1, 2, 3], [0, 0.5, np.inf], [-2.5, 7.0]):
        st, msg = _transient_device(edges, len(edges) - 1, frame=C.c_void_p(16), bins=C.c_void_p(16))
        assert st == INVALID_ARGUMENT and "transient film" not in msg and "NULL" in msg, msg
    # the synchronous form checks the edges first as well
    L = device.lib()
    e = np.array([0, 2, 1], np.float32)
    st = L.wpt_render_transient_block(None, None, None, C.c_void_p(e.ctypes.data), 2, 16, 16, 1, 0, 256, None, None)
    assert st == INVALID_ARGUMENT and "increase" in L.wpt_last_error().decode()
    e = np.array([0, 2, 3], np.float32)
    st = L.wpt_render_transient_block(None, None, None, C.c_void_p(e.ctypes.data), 2, 16, 16, 1, 0, 256, None, None)
    assert st == INVALID_ARGUMENT and "block_bins" in L.wpt_last_error().decode()


def test_transient_entry_points_are_exported_and_declared():
    L = device.lib()
    for name in ("wpt_render_transient_block_device", "wpt_render_transient_block"):
        assert name in device.EXPORTS
        getattr(L, name)
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    assert "WPT_TRANSIENT_MAX_BINS 4096u" in header and "#define WPT_ABI_VERSION 5u" in header
    assert _abi.WPT_ABI_VERSION == 5
    # the transient kernels are units of their own in the library's build
    makefile = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read()
    for unit in ("wpt_k_basic_lds_transient", "wpt_k_full_transient", "wpt_k_full_anim_transient", "wpt_k_full_rgl_anim_transient"):
        assert unit in makefile.split()  # the list of units, one name per line
