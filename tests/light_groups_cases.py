"""What the light-groups tests share: the fixture scenes (32 x 24, 9 samples per pixel, max_path_components = 8), a scene's
emitters and its muted twins, the feature bits the library finds in a scene, and the derived bound of the planes' sum."""
import functools

import numpy as np

from wurblpt_amd import _abi, host

W, H, S, MAX_PATH = 32, 24, 3, 8
NONE = _abi.LIGHT_GROUP_NONE

# name -> (constructor for a size, exposure interval or None)
SCENES = {
    "variant0": (lambda w, h: host.light_groups_scene(w, h, 0), None),
    "variant1": (lambda w, h: host.light_groups_scene(w, h, 1), None),
    "variant2": (lambda w, h: host.light_groups_scene(w, h, 2, 0.0, 1.0), (0.0, 1.0)),
    "variant3": (lambda w, h: host.light_groups_scene(w, h, 3), None),
    "spot_stage": (lambda w, h: host.spot_scene(w, h, 1), None),
    "spheres": (lambda w, h: host.spheres(w, h, 0), None),
    "mis_test": (lambda w, h: host.mis_test(w, h), None),
}
# further scenes of the GPU tests (no CPU renders of them)
SCENES_GPU = {
    "variant0_dispersive": (lambda w, h: host.light_groups_scene(w, h, 0, dispersive=True), None),
}
# the transient kernel each fixture must run on (wpt_kernel_table.h): all four are covered
KERNEL_OF = {
    "variant0": "wpt_pathtrace, transient, scene in LDS",
    "variant1": "wpt_pathtrace, transient, all features",
    "variant2": "wpt_pathtrace, transient, all features, moving scenes",
    "variant3": "wpt_pathtrace, transient, measured BRDFs",
}


def make(name, w=W, h=H):
    return {**SCENES, **SCENES_GPU}[name][0](w, h)


def params(name=None, **gates):
    p = host.default_params()
    p.max_path_components = MAX_PATH
    times = {**SCENES, **SCENES_GPU}[name][1] if name is not None else None
    if times is not None:
        p.t0, p.t1 = times
    for k, v in gates.items():
        setattr(p, k, v)
    return p


def sources(sc):
    """the scene's emitters in the tests' order: its emitting material records, then "env" where it has an environment"""
    return list(host.emitters(sc)) + (["env"] if sc.d.envmap.type != 0 else [])


def table(sc, groups):
    """the launch's table and environment group for `groups`: a list of lists of sources; what is in no list has group NONE"""
    t = np.full(sc.d.material_count, NONE, np.uint8)
    env = NONE
    for g, members in enumerate(groups):
        for m in members:
            if m == "env":
                env = g
            else:
                t[m] = g
    return t, env


def twin(name, keep, w=W, h=H):
    """the muted twin: the same description in which only the sources in `keep` emit"""
    sc = make(name, w, h)
    host.mute_emitters(sc, [k for k in keep if k != "env"])
    if "env" not in keep:
        host.mute_environment(sc)
    return sc


def need(sc, p):
    """the feature bits the library finds in a scene and a launch (sceneFeatures, wpt_capi_scene.hip, and renderLaunch, wpt_capi_render.hip)"""
    TEXTURES, MODPHONG, ENVMAP, LENS, TWOSIDED, GGX, GLASS, SPHERES, RGL, ANIM, SPOT = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 2048
    d = sc.d
    f = 0
    for i in range(d.material_count):
        m = d.materials[i]
        f |= {_abi.MAT_MODPHONG: MODPHONG, _abi.MAT_TWOSIDED: TWOSIDED, _abi.MAT_GGX: GGX, _abi.MAT_GLASS: GLASS, _abi.MAT_MIRROR: GLASS,
              _abi.MAT_LIGHT_SPOT: SPOT, _abi.MAT_RGL: RGL}.get(m.type, 0)
        if m.normal_tex >= 0 or (m.type != _abi.MAT_TWOSIDED and any(t >= 0 for t in m.tex)):
            f |= TEXTURES
    if d.envmap.type != 0:
        f |= ENVMAP | TEXTURES
    if d.sphere_count > 0:
        f |= SPHERES
    if any(d.instances[i].animation >= 0 for i in range(d.instance_count)) or any(d.spheres[i].animation >= 0 for i in range(d.sphere_count)):
        f |= ANIM
    cam = sc.camera.contents
    if cam.lens_radius > 0.0:
        f |= LENS
    if p.t0 != p.t1 or cam.animation >= 0:
        f |= ANIM
    return f


def sum_bound(max_path_components, samples_sqrt):
    """|sum of planes - frame| <= 2 (m + 1) u * frame: all terms are non-negative, u = 2^-24, and a pixel's frame sum and its
    plane sums each make at most m = 2 * max_path_components * n^2 additions plus one scaling"""
    m = 2 * max_path_components * samples_sqrt * samples_sqrt
    return 2.0 * (m + 1) * 2.0 ** -24


def check_sum(planes, frame, bound):
    """the planes, summed in float64, against the frame: within bound * frame in every value (so 0 where the frame is 0)"""
    total = np.asarray(planes, np.float64).sum(axis=0)
    f = frame.astype(np.float64)
    err = np.abs(total - f)
    rel = float((err[f > 0] / f[f > 0]).max()) if (f > 0).any() else 0.0
    print("planes' sum against the frame: largest relative difference %.3g (bound %.3g)" % (rel, bound))
    assert (err <= bound * f).all(), rel
    return rel


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """(full frame, its counters, {source: (twin frame, its counters)}) from the CPU restatement, computed once"""
    from tests import oracle_loader
    o = oracle_loader.load("portable")
    p = params(name)
    sc = make(name)
    full, counters = o.render(sc, S, params=p)
    twins = {}
    for src in sources(sc):
        twins[src] = o.render(twin(name, [src]), S, params=p)
    for a in [full] + [t[0] for t in twins.values()]:
        a.setflags(write=False)
    return full, counters, twins
