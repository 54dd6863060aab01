"""LightSpot (light_spot.hpp) without a GPU: the C++ class flattens to a LIGHT_SPOT record with the reference's values, the
host scenes that use it carry it where the reference puts it, upload validation accepts it and checks its texture, and the
example application builds against the public headers and stops without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")

RECORD_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <wurblpt/wurblpt.hpp>
using namespace WurblPT;
static void print(const wpt_material& m)
{
    unsigned int b[5];
    memcpy(b, m.v[0], 16);
    memcpy(b + 4, m.f, 4);
    printf("%u %d %d %08x %08x %08x %08x %08x\n", m.type, m.tex[0], m.normal_tex, b[0], b[1], b[2], b[3], b[4]);
}
int main(int argc, char* argv[])
{
    /* argv: angle r g b; prints LightSpot, LightSpot with a texture, LightDiffuse of the same emission */
    if (argc != 5)
        return 2;
    const float angle = strtof(argv[1], nullptr);
    const vec3 emit(strtof(argv[2], nullptr), strtof(argv[3], nullptr), strtof(argv[4], nullptr));
    TextureChecker checker(vec3(1.0f), vec3(0.0f));
    FlattenContext ctx;
    wpt_material m;
    if (!LightSpot(angle, emit).describe(m, ctx))
        return 1;
    print(m);
    if (!LightSpot(angle, emit, &checker).describe(m, ctx))
        return 1;
    print(m);
    if (!LightDiffuse(emit).describe(m, ctx))
        return 1;
    print(m);
    return 0;
}
"""


def compile_cpp(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def cosf(x):
    libm = C.CDLL("libm.so.6")
    libm.cosf.restype = C.c_float
    libm.cosf.argtypes = [C.c_float]
    return np.float32(libm.cosf(np.float32(x)))


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def test_abi_value():
    assert _abi.MAT_LIGHT_SPOT == 9


def test_light_spot_record_has_the_reference_values(tmp_path):
    """type 9, f[0] = cosf(0.5f * openingAngle) bit for bit, v[0] = (rgb, average(rgb)) as LightDiffuse(vec3) has it,
    tex[0] the emission texture or -1"""
    src = tmp_path / "record.cpp"
    src.write_text(RECORD_PROGRAM)
    exe = compile_cpp(tmp_path, str(src), "record")
    cases = [(0.5235988, 4.0, 4.0, 4.0), (1.3, 0.3, 2.5, 7.0), (2 * np.pi, 1.0, 0.5, 0.25), (0.01, 9.0, 0.0, 1.0), (4.5, 1.0, 2.0, 3.0)]
    for angle, r, g, b in cases:
        angle = np.float32(angle)
        out = subprocess.run([exe, repr(float(angle)), repr(r), repr(g), repr(b)], capture_output=True, check=True, timeout=60)
        spot, spot_tex, diffuse = [line.split() for line in out.stdout.decode().split("\n")[:3]]
        assert spot[0] == "9" and spot[1] == "-1" and spot[2] == "-1"
        assert int(spot[7], 16) == f32_bits(cosf(np.float32(0.5) * angle)), (angle, spot)
        assert spot[3:7] == diffuse[3:7]                                   # (r, g, b, average) as LightDiffuse(vec3)
        assert [int(x, 16) for x in spot[3:6]] == [f32_bits(r), f32_bits(g), f32_bits(b)]
        assert spot_tex[0] == "9" and spot_tex[1] == "0" and spot_tex[3:] == spot[3:]
    # the full circle: cos(pi) = -1 exactly, every direction is inside the cone
    assert cosf(np.float32(0.5) * np.float32(2 * np.pi)) == -1.0


def _materials(sc):
    return [sc.d.materials[i] for i in range(sc.d.material_count)]


def test_cornell_spot_scene_is_the_applications_third_light():
    """MaterialTwoSided(LightSpot(radians(30), vec3(4)), MaterialLambertian(vec3(0))) on the ceiling light, which stays
    the only hot spot"""
    sc = host.spot_scene(32, 24, 0)
    mats = _materials(sc)
    two = [m for m in mats if m.type == _abi.MAT_TWOSIDED]
    assert len(two) == 1
    front, back = mats[two[0].tex[0]], mats[two[0].tex[1]]
    assert front.type == _abi.MAT_LIGHT_SPOT and back.type == _abi.MAT_LAMBERTIAN
    assert list(front.v[0]) == [4.0, 4.0, 4.0, 4.0] and front.tex[0] == -1
    assert f32_bits(front.f[0]) == f32_bits(cosf(np.float32(0.5) * np.float32(30.0) * (np.float32(np.pi) / np.float32(180.0))))
    assert list(back.v[0])[:3] == [0.0, 0.0, 0.0]
    assert sc.d.hotspot_count == 2
    light = next(i for i in range(len(mats)) if mats[i].type == _abi.MAT_TWOSIDED)
    assert all(sc.d.tri_geom[sc.d.hotspots[k].prim].material == light for k in range(sc.d.hotspot_count))
    plain = host.cornell(32, 24, 0, 0)
    assert plain.d.tri_count == sc.d.tri_count and plain.d.node_count == sc.d.node_count


def test_stage_scene_has_coloured_spots_a_gobo_and_a_spherical_spot():
    sc = host.spot_scene(32, 24, 1)
    mats = _materials(sc)
    spots = [m for m in mats if m.type == _abi.MAT_LIGHT_SPOT]
    assert len(spots) == 4
    assert sum(m.tex[0] >= 0 for m in spots) == 1                        # the checker-textured one
    assert len({tuple(m.v[0]) for m in spots}) == 4                      # each its own colour
    assert len({float(m.f[0]) for m in spots}) == 4                      # and its own opening angle
    spheres = [sc.d.spheres[i] for i in range(sc.d.sphere_count)]
    assert any(mats[s.material].type == _abi.MAT_LIGHT_SPOT for s in spheres)
    kinds = sorted(sc.d.hotspots[k].kind for k in range(sc.d.hotspot_count))
    assert kinds == [0] * 6 + [1]                                         # three lamp quads and the lamp sphere


def _upload_status(sc):
    handle = C.c_void_p()
    st = device.lib().wpt_scene_upload(sc.desc, C.byref(handle))
    if st == 0 and handle.value:        # only where a GPU is present
        device.lib().wpt_scene_free(handle)
    return st, device.lib().wpt_last_error().decode()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_upload_validation_accepts_spot_records(variant):
    st, message = _upload_status(host.spot_scene(16, 16, variant))
    assert st == 0 or "no HIP device" in message or "no ROCm" in message, message


def test_upload_validation_refuses_a_spot_texture_outside_the_array():
    sc = host.spot_scene(16, 16, 1)
    spot = next(m for m in _materials(sc) if m.type == _abi.MAT_LIGHT_SPOT)
    spot.tex[0] = sc.d.texture_count
    st, message = _upload_status(sc)
    assert st == 1 and "texture" in message.lower(), (st, message)


def test_upload_validation_still_refuses_unknown_types():
    sc = host.spot_scene(16, 16, 0)
    for t in (10, 99):
        sc.d.materials[0].type = t
        st, message = _upload_status(sc)
        assert st == 4 and "material type" in message, (t, st, message)


def test_stage_lights_example_builds_and_needs_a_device(tmp_path):
    """One include (<wurblpt/wurblpt.hpp>) and one library, -Wall -Wextra -Werror; without a GPU the program says so and
    stops, nothing is rendered on the CPU"""
    import torch
    exe = compile_cpp(tmp_path, os.path.join(ROOT, "examples", "stage_lights.cpp"), "stage_lights")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the run is covered by the gpu test")
    r = subprocess.run([exe, "16", "12", "1", str(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"no HIP device" in r.stderr
    assert not os.path.exists(str(tmp_path / "stage.png"))
