"""Light groups (SensorRGBLightGroups, wpt_render_light_groups_block*, wpt_postproc_mix_planes*) without a GPU: bad tables are
refused before a device is needed, the entry points are exported and declared, the host mix is numpy's float32 evaluation of the
same expression bit for bit, wpt_lightmix.h stands on its own under the sanitizers, the C++ sensor resolves its assignments to the
flattened records, and -- with the CPU restatement -- muting emitters changes no path: every muted twin of the fixture scenes does
the full scene's work, and the twins add up to the full frame within the derived bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import light_groups_cases as cases
from wurblpt_amd import _abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wurblpt_amd", "lib")
INVALID_ARGUMENT = 1
NONE = _abi.LIGHT_GROUP_NONE


def _launch(table, material_count, group_count, env_group, scene=None, frame=None, planes=None, synchronous=False):
    L = device.lib()
    arr = None if table is None else np.ascontiguousarray(table, dtype=np.uint8)
    ptr = None if arr is None else C.c_void_p(arr.ctypes.data)
    if synchronous:
        st = L.wpt_render_light_groups_block(scene, None, None, ptr, material_count, group_count, env_group, 16, 16, 1, 0, 256, frame, planes)
    else:
        st = L.wpt_render_light_groups_block_device(scene, None, None, ptr, material_count, group_count, env_group, 16, 16, 1, 0, 256,
                                                    frame, planes, None)
    return st, L.wpt_last_error().decode()


def test_bad_tables_are_refused_without_a_device():
    some = C.c_void_p(16)
    bad = [(None, 4, 2, 0, "NULL"), ([0, 1], 2, 0, 0, "group count"), ([0, 1], 2, 256, 0, "group count"), ([0, 1, 2], 3, 2, 0, "material 2"),
           ([0, 254, 0], 3, 254, 0, "material 1"), ([3, 0], 2, 3, NONE, "material 0"), ([0, 1], 2, 2, 2, "environment"),
           ([0, NONE], 2, 1, 1, "environment"), ([0, 0], 2, 1, 0x1ff, "environment")]
    for table, count, K, env, what in bad:
        for synchronous in (False, True):
            st, msg = _launch(table, count, K, env, frame=some, planes=some, synchronous=synchronous)
            assert st == INVALID_ARGUMENT and "light groups" in msg and what in msg, (table, K, env, msg)
    # a good table passes the check: what is refused then is the missing scene (or, in the synchronous form, the missing planes)
    for table, K, env in (([0, 1, NONE, 1], 2, 0), ([0] * 7, 1, NONE), ([254, NONE, 0], 255, 254), ([NONE, NONE], 3, NONE)):
        st, msg = _launch(table, len(table), K, env, frame=some, planes=some)
        assert st == INVALID_ARGUMENT and "light groups" not in msg and "NULL" in msg, msg
        st, msg = _launch(table, len(table), K, env, synchronous=True)
        assert st == INVALID_ARGUMENT and "block_planes" in msg, msg
    # no entry of an empty table is read
    st, msg = _launch([], 0, 1, 0, frame=some, planes=some)
    assert st == INVALID_ARGUMENT and "light groups" not in msg


def test_entry_points_are_exported_and_declared():
    L = device.lib()
    header = open(os.path.join(ROOT, "include", "wurblpt_hip.h")).read()
    names = ("wpt_render_light_groups_block_device", "wpt_render_light_groups_block", "wpt_postproc_mix_planes", "wpt_postproc_mix_planes_host")
    for name in names:
        assert name in device.EXPORTS and not re.search(r"\d", name)
        getattr(L, name)
        assert re.search(r"wpt_status %s\(" % name, header)
    assert "#define WPT_LIGHT_GROUPS_MAX 255u" in header and "#define WPT_LIGHT_GROUP_NONE 0xffu" in header
    assert "#define WPT_ABI_VERSION 5u" in header and _abi.WPT_ABI_VERSION == 5
    assert (_abi.LIGHT_GROUPS_MAX, _abi.LIGHT_GROUP_NONE) == (255, 0xff)
    # a light-groups launch is a launch of the transient film's kernels: no unit, no table row and no sensor of its own
    makefile = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "Makefile")).read()
    assert not any("group" in unit for unit in makefile.split() if unit.startswith("wpt_k_"))
    assert not any("group" in name for _, name in device.kernel_table())
    blocks = open(os.path.join(ROOT, "wurblpt_amd", "csrc", "wpt_blocks.h")).read()
    assert "uint32_t rule;" in blocks


@pytest.mark.parametrize("K", [1, 3, 17])
def test_host_mix_is_numpys_float32_expression(K):
    rng = np.random.RandomState(100 + K)
    planes = (rng.rand(K, 7, 5, 3) * 4).astype(np.float32)
    planes[rng.rand(*planes.shape) < 0.1] = 0.0
    planes[0, 0, 0] = np.float32(1e-42)                                    # a denormal value under a weight below 1
    weights = (rng.rand(K, 3) * 2).astype(np.float32)
    weights[0] = [-1.5, 0.0, np.float32(1e-40)]                              # negative, zero and denormal
    if K > 1:
        weights[K // 2] = [np.float32(-1e-41), -0.0, 0.25]
        weights[K - 1, 0] = -weights[K - 1, 0]
    got = device.mix_planes_host(planes, weights)
    acc = np.zeros(planes.shape[1:], np.float32)
    for k in range(K):
        acc = acc + (weights[k] * planes[k]).astype(np.float32)             # ((0 + w0 P0) + w1 P1) + ..., one rounding per operation
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), acc.view(np.uint32))
    assert np.isfinite(got).all() and ((got < 0).any() or K > 3)         # the negative weights show where few planes outweigh them
    # one weight per plane stands for all three channels; planes further apart than their pixels are read where they are
    assert np.array_equal(device.mix_planes_host(planes, weights[:, 1]), device.mix_planes_host(planes, np.repeat(weights[:, 1:2], 3, axis=1)))
    wide = np.zeros((K, 7 * 5 * 3 + 9), np.float32)
    wide[:, :7 * 5 * 3] = planes.reshape(K, -1)
    out = np.zeros(7 * 5 * 3, np.float32)
    w = np.ascontiguousarray(weights)
    st = device.lib().wpt_postproc_mix_planes_host(C.c_void_p(wide.ctypes.data), K, wide.shape[1], 35, C.c_void_p(w.ctypes.data),
                                                   C.c_void_p(out.ctypes.data))
    assert st == 0 and np.array_equal(out.view(np.uint32), acc.reshape(-1).view(np.uint32))


def test_bad_mixes_are_refused():
    L = device.lib()
    a = np.zeros(64, np.float32)
    p = C.c_void_p(a.ctypes.data)
    for args, what in (((None, 1, 12, 4, p, p), "NULL"), ((p, 0, 12, 4, p, p), "plane count"), ((p, 4097, 12, 4, p, p), "plane count"),
                       ((p, 2, 11, 4, p, p), "overlap"), ((p, 1, 12, 0, p, p), "pixel count")):
        assert L.wpt_postproc_mix_planes_host(*args) == INVALID_ARGUMENT and what in L.wpt_last_error().decode(), args
        assert L.wpt_postproc_mix_planes(*args, None) == INVALID_ARGUMENT and what in L.wpt_last_error().decode(), args


def test_the_mix_and_the_table_check_on_their_own_under_the_sanitizers(tmp_path):
    """tests/lightmix_check.cpp: wpt_lightmix.h without the library or a header of HIP, every buffer of the promised size"""
    exe = str(tmp_path / "lightmix_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "lightmix_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-3000:]
    assert not r.stderr, r.stderr.decode()[-2000:]
    words = out.strip().splitlines()[-1].replace("(", " ").split()
    assert "BROKEN" not in out and words[-2:] == ["0", "failures"]
    mixes, tables, refused = int(words[0]), int(words[2]), int(words[4])
    assert mixes >= 3000 and tables >= 200000 and tables // 4 <= refused <= tables // 2, out


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_muting_emitters_changes_no_path_and_the_twins_add_up(name):
    """the CPU restatement at 32 x 24, 9 spp, max_path_components = 8: for every emitter kept alone (the environment among them
    where there is one) the work counters are the full scene's; frames and twins are finite and not negative; every twin is lit
    somewhere and no two are alike; and the twins sum to the frame within 2 (m + 1) u * frame, m = 2 * 8 * 9"""
    full, counters, twins = cases.oracle_frames(name)
    sc = cases.make(name)
    srcs = cases.sources(sc)
    assert len(srcs) >= 2 and list(twins) == srcs
    assert counters["samples"] == cases.W * cases.H * cases.S * cases.S and counters["scatters"] > 0
    assert np.isfinite(full).all() and (full >= 0).all() and full.any()
    for src, (frame, c) in twins.items():
        assert c == counters, (src, c, counters)
        assert np.isfinite(frame).all() and (frame >= 0).all(), src
        assert (frame > 0).any(), "twin %s is dark" % src
    for i, a in enumerate(srcs):
        for b in srcs[i + 1:]:
            assert not np.array_equal(twins[a][0], twins[b][0]), (a, b)
    bound = cases.sum_bound(cases.MAX_PATH, cases.S)
    assert abs(bound - 1.7e-5) < 0.1e-5                                     # 2 * 145 * 2^-24
    cases.check_sum([t[0] for t in twins.values()], full, bound)
    # the kept-alone scene has exactly the kept emitter left
    for src in srcs:
        left = cases.sources(cases.twin(name, [src]))
        assert [s for s in left if s != "env"] == [s for s in [src] if s != "env"]


def test_fixture_scenes_are_what_the_launch_forms_need():
    """variant 0: Lambertian, GGX, glass and diffuse lamps only, small enough for LDS; 1: a two-sided spot, a ModPhong panel with an
    emission texture, a sphere lamp and an equirect environment without tables, with hot spots; 2: animated; 3: measured BRDFs"""
    T = _abi
    sc = cases.make("variant0")
    types = [sc.d.materials[i].type for i in range(sc.d.material_count)]
    assert set(types) == {T.MAT_LAMBERTIAN, T.MAT_GGX, T.MAT_GLASS, T.MAT_LIGHT_DIFFUSE} and types.count(T.MAT_LIGHT_DIFFUSE) == 2
    assert cases.need(sc, cases.params("variant0")) == 32 | 64 and sc.d.envmap.type == 0 and sc.d.texture_count == 0
    for name in cases.KERNEL_OF:
        sc = cases.make(name)
        d = sc.d
        chosen = device.kernel_choice(cases.need(sc, cases.params(name)), device.SENSOR_TRANSIENT, False, d.node_count, d.tri_count, d.material_count)
        assert chosen[0] == cases.KERNEL_OF[name], (name, chosen)
    sc = cases.make("variant1")
    d = sc.d
    types = [d.materials[i].type for i in range(d.material_count)]
    assert {T.MAT_TWOSIDED, T.MAT_LIGHT_SPOT, T.MAT_MODPHONG} <= set(types) and d.sphere_count == 1 and d.hotspot_count > 0
    assert d.envmap.type == 1 and d.envmap.N == 0
    panel = [d.materials[i] for i in host.emitters(sc) if d.materials[i].type == T.MAT_MODPHONG]
    assert len(panel) == 1 and panel[0].tex[4] >= 0
    assert len(cases.sources(sc)) == 6
    dispersive = host.light_groups_scene(32, 24, 0, dispersive=True)
    glass = [dispersive.d.materials[i] for i in range(dispersive.d.material_count) if dispersive.d.materials[i].type == T.MAT_GLASS]
    assert len(glass) == 1 and glass[0].flags & 2                          # WPT_MATF_CHROMATIC_DISPERSION
    with pytest.raises(ValueError):
        host.mute_environment(host.sponza_like(16, 12, detail=0.02, tex_size=8, env_width=16, importance_n=4))


SENSOR_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <wurblpt/wurblpt.hpp>
using namespace WurblPT;
int main()
{
    int refused = 0;
    for (unsigned int k : { 0u, 256u, 1000u }) {
        try { SensorRGBLightGroups s(4, 3, k); } catch (const std::invalid_argument&) { refused++; }
    }
    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.7f)));
    Material* lampA = scene.take(new LightDiffuse(vec3(1.0f)));
    Material* lampB = scene.take(new LightDiffuse(vec3(2.0f)));
    Material* front = scene.take(new LightSpot(radians(40.0f), vec3(3.0f)));
    Material* back = scene.take(new MaterialLambertian(vec3(0.0f)));
    Material* spot = scene.take(new MaterialTwoSided(front, back));
    Material* lampC = scene.take(new LightDiffuse(vec3(4.0f)));
    for (Material* m : { white, lampA, lampB, spot, lampC })
        scene.take(new MeshInstance(scene.take(generateQuad()), m));
    scene.updateBVH();
    SensorRGBLightGroups s(4, 3, 4, 0.5f, 9.0f, 1.0f, 7.0f);
    try { s.assign(lampA, 4); } catch (const std::invalid_argument&) { refused++; }
    try { s.assignEnvironment(4); } catch (const std::invalid_argument&) { refused++; }
    s.assign(lampA, 1);
    s.assign(lampB, 2);
    s.assign(spot, 3);
    s.assignEnvironment(2);
    FlatScene flat;
    if (!scene.flatten(flat))
        return 1;
    const std::vector<uint8_t> table = lightGroupsTable(s, scene, flat);
    printf("%d %u %u %zu %zu %g %g %g %g\n", refused, s.groupCount(), s.environmentGroup(), s.group(3).dimension(0), s.group(0).dimension(1),
            s.minDistToLight, s.maxDistToLight, s.minPathLen, s.maxPathLen);
    for (size_t i = 0; i < table.size(); i++)
        printf("%u:%u ", flat.materials[i].type, unsigned(table[i]));
    printf("\n");
    /* the mix of the (empty) groups needs no device */
    const Array<float> mixed = mixLightGroups(s, std::vector<float>(12, 0.5f));
    try { mixLightGroups(s, std::vector<float>(11, 0.5f)); } catch (const std::invalid_argument&) { printf("weights refused\n"); }
    printf("%zu %zu\n", mixed.dimension(0), mixed.dimension(1));
    return 0;
}
"""


def compile_cpp(tmp_path, source, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++20", "-O1", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), source,
           "-L" + LIB, "-lwurblpt_hip", "-Wl,-rpath," + LIB, "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


def test_sensor_resolves_its_assignments_to_the_flattened_records(tmp_path):
    src = tmp_path / "sensor.cpp"
    src.write_text(SENSOR_PROGRAM)
    exe = compile_cpp(tmp_path, str(src), "sensor")
    out = subprocess.run([exe], capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert out[0].split() == ["5", "4", "2", "4", "3", "0.5", "9", "1", "7"]
    T = _abi
    records = [tuple(int(x) for x in w.split(":")) for w in out[1].split()]
    by_type = {}
    for t, g in records:
        by_type.setdefault(t, []).append(g)
    # lamps A, B, C in the order of their first use: groups 1, 2 and (unassigned) 0; the two-sided lamp gives 3 to both children
    assert by_type[T.MAT_LIGHT_DIFFUSE] == [1, 2, 0] and by_type[T.MAT_LIGHT_SPOT] == [3] and by_type[T.MAT_TWOSIDED] == [3]
    assert sorted(by_type[T.MAT_LAMBERTIAN]) == [0, 3]                       # the wall (unassigned) and the lamp's black back
    assert out[2] == "weights refused" and out[3].split() == ["4", "3"]


def test_light_mixer_example_builds_and_needs_a_device(tmp_path):
    import torch
    exe = compile_cpp(tmp_path, os.path.join(ROOT, "examples", "light_mixer.cpp"), "light_mixer")
    if not torch.cuda.is_available():       # (with a device the run is tests/test_gpu_light_groups.py's)
        r = subprocess.run([exe, "16", "12", "1", str(tmp_path)], capture_output=True, timeout=120)
        assert r.returncode != 0 and b"no HIP device" in r.stderr
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".pfm")]          # nothing is faked on the CPU
