"""The C++ interface of temporal accumulation (WurblPT::TemporalAccumulator, include/wurblpt/postproc.hpp) without a GPU:
tests/temporal_cpp_api.cpp drives it over three synthetic frames and checks every result against the C host form; the digests
it prints are those of the Python host form on arrays made again here."""
import os
import subprocess

import numpy as np

from tests import denoise_cases as cases
from wurblpt_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cpp_interface_gives_the_host_forms_bits(tmp_path):
    lib = os.path.join(ROOT, "wurblpt_amd", "lib")
    exe = str(tmp_path / "temporal_cpp_api")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "temporal_cpp_api.cpp"), "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
    w, h = 20, 11
    i = np.arange(w * h)
    x, y = i % w, i // w
    m = ((x // 4 + y // 3) % 3 - 1).astype(np.int32)
    n_p = (i % 4).reshape(h, w)
    normals = np.zeros((w * h, 3), np.float32)
    normals[m >= 0, 2] = 1
    positions = np.where((m >= 0)[:, None], np.stack([x / 32.0, y / 32.0, -2.0 - 0.5 * m], axis=1), 0).astype(np.float32)
    shaped = lambda a: a.reshape(h, w, -1)
    guide = (shaped(positions), shaped(normals), m.reshape(h, w))
    pixel = np.broadcast_to(np.array([-0.25, 0.5], np.float32), (h, w, 2)).copy()
    camera = np.broadcast_to(np.array([-0.25 / 32, 0.5 / 32, 0], np.float32), (h, w, 3)).copy()
    history = None
    for k in range(3):
        frame = np.where((n_p.reshape(-1) == 0)[:, None], 0, ((i[:, None] * 7 + np.arange(3) * 3 + k * 5) % 16) / 8.0).astype(np.float32)
        moments = (frame * frame * np.float32(1.5)).astype(np.float32)
        history = device.temporal_accumulate_host(shaped(frame), shaped(moments), n_p, guide, (pixel, camera) if k == 2 else None, history,
                                                  device.temporal_params(max_history=2))
    out, var = device.denoise_history_host(history, _abi.DenoiseParams(iterations=3), True)
    assert r.stdout.decode().split() == [cases.digest(history), cases.digest(out), cases.digest(var), "kept"]
    N = history[1, ..., 3]
    assert N.max() == 2 and (N == 1).any() and (N == 0).any()   # kept up to max_history, reset (the sky), never sampled
