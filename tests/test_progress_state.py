"""Progressive sessions without a device: the C ABI's new entry points exist, wpt_progress_begin says that there is no device,
the saved state's header is parsed as include/wurblpt_hip.h documents it -- by the library on states this file writes from
that table, and by the parser on its own under the sanitizers -- and the scene's tag is the documented hash."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wpt_progress_covers", "wpt_progress_begin", "wpt_progress_advance_device", "wpt_progress_advance", "wpt_progress_rows_done",
         "wpt_progress_rows_total", "wpt_progress_preview_device", "wpt_progress_preview", "wpt_progress_end", "wpt_progress_state_bytes",
         "wpt_progress_save", "wpt_progress_restore", "wpt_progress_state_info"]

# the layout, written down here from the table in include/wurblpt_hip.h (not taken from the package)
HEADER = 224
FIELDS = [("magic", 0, 4), ("version", 4, 4), ("width", 8, 4), ("height", 12, 4), ("samples_sqrt", 16, 4), ("block_start", 20, 4),
          ("block_size", 24, 4), ("rows_done", 28, 4), ("tag", 32, 8), ("camera", 40, 140), ("params", 180, 40), ("reserved", 220, 4)]


def make_state(width=7, height=5, samples_sqrt=6, block_start=3, block_size=29, rows_done=2, tag=0x0123456789abcdef, magic=0x50545057, version=1,
               carry=None):
    head = struct.pack("<8IQ", magic, version, width, height, samples_sqrt, block_start, block_size, rows_done, tag)
    head += bytes([0x11]) * 140 + bytes([0x22]) * 40 + bytes(4)
    assert len(head) == HEADER
    return head + (bytes([0x33]) * (32 * block_size) if carry is None else carry)


def refusal(state):
    with pytest.raises(RuntimeError) as e:
        device.progress_state_info(state)
    assert "(status 1)" in str(e.value), str(e.value)       # WPT_ERR_INVALID_ARGUMENT
    return str(e.value)


def test_the_entry_points_are_declared_in_plain_c_and_exported():
    text = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    L = device.lib()
    for name in NAMES:
        assert name + "(" in text, name
        assert name in device.EXPORTS and hasattr(L, name), name
    assert _abi.PROGRESS_HEADER_BYTES == HEADER and C.sizeof(_abi.ProgressInfo) == 48
    assert "#define WPT_PROGRESS_HEADER_BYTES 224u" in text and "#define WPT_PROGRESS_MAGIC 0x50545057u" in text


def test_begin_without_a_device_says_so():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    sc = host.cornell(16, 16)
    handle = C.c_void_p(1)
    p = host.default_params()
    st = device.lib().wpt_progress_begin(None, sc.camera, C.byref(p), 16, 16, 4, 0, 256, 0, C.byref(handle))
    assert st == 2 and not handle.value                     # WPT_ERR_NO_DEVICE
    assert b"no HIP device" in device.lib().wpt_last_error()


def test_what_sessions_do_not_cover_is_refused_with_its_reason():
    device.progress_covers()
    for kwargs, word in [(dict(sensor=device.SENSOR_TRANSIENT), "transient"), (dict(sensor=device.SENSOR_VIEWS), "views"),
                         (dict(sensor=device.SENSOR_ADAPTIVE), "adaptive"), (dict(sensor=device.SENSOR_TOF), "time-of-flight"),
                         (dict(counting=True), "counting"), (dict(bands=True), "bands")]:
        with pytest.raises(RuntimeError, match=word) as e:
            device.progress_covers(**kwargs)
        assert "(status 4)" in str(e.value)                 # WPT_ERR_UNSUPPORTED


def test_state_info_reads_a_state_written_from_the_documented_layout():
    info = device.progress_state_info(make_state())
    assert info == dict(version=1, width=7, height=5, samples_sqrt=6, block_start=3, block_size=29, rows_done=2, tag=0x0123456789abcdef,
                        state_bytes=HEADER + 32 * 29)
    assert device.progress_state_info(make_state(rows_done=6))["rows_done"] == 6      # a finished session's state
    assert device.progress_state_info(make_state(65535, 65535, 65535, 65535 * 65535 - 1, 1, 0, carry=bytes(32)))["block_size"] == 1


def test_state_info_refuses_each_bad_state_with_its_own_message():
    good = make_state()
    messages = {}
    for name, offset, size in FIELDS:
        for cut in (offset, offset + size - 1):
            m = refusal(good[:cut])
            assert "ends within" in m and (name in m), (name, cut, m)
            messages["cut in " + name] = m
    messages["header only"] = refusal(good[:HEADER])
    assert messages["header only"] == refusal(good[:-1]) and "carry" in messages["header only"]
    messages["too long"] = refusal(good + b"\0")
    messages["magic"] = refusal(make_state(magic=0x50545058))
    assert "magic" in messages["magic"]
    messages["version"] = refusal(make_state(version=2))
    assert "version" in messages["version"]
    messages["block"] = refusal(make_state(block_size=33))            # 3 + 33 > 7 * 5
    assert "block" in messages["block"] and messages["block"] == refusal(make_state(block_start=0xfffffff0))
    messages["rows"] = refusal(make_state(rows_done=7))
    assert "rows_done" in messages["rows"]
    messages["range"] = refusal(make_state(samples_sqrt=0))
    messages["reserved"] = refusal(good[:220] + b"\1\0\0\0" + good[224:])
    assert "reserved" in messages["reserved"]
    assert len(set(messages.values())) == len(messages), messages
    # and the library's entry point itself wants an `info` to fill
    assert device.lib().wpt_progress_state_info(good, len(good), None) == 1


def test_the_parser_on_its_own_under_the_sanitizers(tmp_path):
    """tests/progress_state_check.cpp: the header parser compiled outside the library with -fsanitize=address,undefined, every
    state in a heap block of exactly its length -- the same cases and 4000 seeded corruptions, no read past `bytes`."""
    exe = str(tmp_path / "progress_state_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "progress_state_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, "4000", "7"], capture_output=True, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-3000:]
    assert "4000 corruptions (seed 7)" in out and ", 0 failures" in out and "EXPECTED" not in out
    assert "rows_done greater than samples_sqrt: the state's rows_done is greater" in out
    assert not r.stderr, r.stderr.decode()[-2000:]


def fnv1a_tag(scene):
    """sceneTag() as include/wurblpt/progressive.hpp documents it, in plain Python"""
    d = scene.d
    arrays = [(d.nodes, d.node_count * 32), (d.tri_geom, d.tri_count * 48), (d.tri_attr, d.tri_count * 96), (d.instances, d.instance_count * 48),
              (d.materials, d.material_count * 128), (d.textures, d.texture_count * 88), (d.texels, d.texel_bytes),
              (d.hotspots, d.hotspot_count * 116), (d.spheres, d.sphere_count * 48), (d.rgl_brdfs, d.rgl_count * 388),
              (d.rgl_data, d.rgl_data_count * 4), (d.animations, d.animation_count * 8), (d.keyframes, d.keyframe_count * 44)]
    data = b""
    for pointer, size in arrays:
        data += struct.pack("<Q", size)
        if size:
            data += C.string_at(C.cast(pointer, C.c_void_p).value, size)
    e = d.envmap
    data += struct.pack("<IIii6i", e.type, e.compat, e.tex, e.N, *e.cube_tex)
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


@pytest.mark.parametrize("make", [lambda: host.cornell(16, 16, 1, 2), lambda: host.animated(16, 16, 8, 0.0, 1.0)], ids=["cornell", "animated"])
def test_scene_tag_is_the_documented_hash_and_sees_one_vertex(make):
    sc = make()
    tag = host.scene_tag(sc)
    assert tag == fnv1a_tag(sc)
    assert tag == host.scene_tag(make()), "the same scene built again has another tag"
    sc.d.tri_geom[sc.d.tri_count // 2].v1[1] = np.nextafter(np.float32(sc.d.tri_geom[sc.d.tri_count // 2].v1[1]), np.float32(9))
    assert host.scene_tag(sc) != tag and host.scene_tag(sc) == fnv1a_tag(sc)
