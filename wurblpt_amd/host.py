"""Host side of the framework for Python callers (tests, bench): scene construction and
flattening through libwurblpt_host.so, which is compiled from the C++ API under
include/wurblpt/ (the mirror of the reference's Scene / Mesh / Material / Camera classes).
CPU only; no HIP dependency."""
import ctypes as C
import os

import numpy as np

from . import _abi

_LIB = None


def lib_path():
    # WPT_LIB_DIR: a second build of the pair of libraries (wurblpt_amd/csrc/Makefile, LIB=...), for experiments
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), os.environ.get("WPT_LIB_DIR", "lib"), "libwurblpt_host.so")


_I, _U, _F, _P, _S, _Q = C.c_int, C.c_uint, C.c_float, C.c_void_p, C.c_char_p, C.c_ulonglong
_SCENE = _P  # wpt_host_scene*: what a scene maker returns and HostScene keeps

# name -> (restype, argtypes) of every function libwurblpt_host.so exports (wurblpt_amd/host/*.cpp), applied by lib();
# tests/test_abi.py holds the table to the library's symbols and to the definitions' parameter counts
FUNCTIONS = {
    "wpt_host_cornell": (_SCENE, [_I, _I, _I, _U, _U]),
    "wpt_host_cornell_checker": (_SCENE, [_U, _U]),
    "wpt_host_random_triangles": (_SCENE, [_U, _U, _I, _U, _U, _F]),
    "wpt_host_lds_edge_scene": (_SCENE, [_U, _U, _I, _U, _U, _U]),
    "wpt_host_sponza_like": (_SCENE, [_U, _F, _U, _U, _I, _U, _U]),
    "wpt_host_courtyard_like": (_SCENE, [_U, _U, _U, _U, _U]),
    "wpt_host_measured_like": (_SCENE, [_U, _F, _U, _U, _I, _S, _S, _U, _U]),
    "wpt_host_animated": (_SCENE, [_I, _F, _F, _U, _U]),
    "wpt_host_furnace": (_SCENE, [_I, _I, _U, _U]),
    "wpt_host_mis_test": (_SCENE, [_I, _U, _U, _U]),
    "wpt_host_texture_probe": (_SCENE, [_I, _U, _U]),
    "wpt_host_spheres": (_SCENE, [_I, _U, _U]),
    "wpt_host_spot_scene": (_SCENE, [_I, _U, _U]),
    "wpt_host_tof_scene": (_SCENE, [_I, _I, _F, _F, _U, _U]),
    "wpt_host_light_groups_scene": (_SCENE, [_I, _F, _F, _S, _S, _U, _U]),
    "wpt_host_rgl_scene": (_SCENE, [_I, _S, _S, _U, _U]),
    "wpt_host_import_obj": (_SCENE, [_S, _U, _F, _F, _F, _P, _P, _F, _U, _U]),
    "wpt_host_import_obj_env": (_SCENE, [_S, _S, _I, _U, _F, _F, _P, _P, _F, _U, _U]),
    "wpt_host_scene_desc": (C.POINTER(_abi.SceneDesc), [_SCENE]),
    "wpt_host_scene_camera": (C.POINTER(_abi.Camera), [_SCENE]),
    "wpt_host_scene_bvh_levels": (_U, [_SCENE]),
    "wpt_host_scene_free": (None, [_SCENE]),
    "wpt_host_scene_set_distortion": (None, [_SCENE, _I, _F, _F, _F, _F, _F]),
    "wpt_host_scene_set_camera_mode": (None, [_SCENE, _I, _F]),
    "wpt_host_scene_material_scene_index": (None, [_SCENE, _P]),
    "wpt_host_scene_tag": (C.c_uint64, [C.POINTER(_abi.SceneDesc)]),
    "wpt_host_default_params": (None, [C.POINTER(_abi.Params)]),
    "wpt_host_bvh_build": (_U, [_U, _P, _P, C.POINTER(_U)]),
    "wpt_host_rgl_build": (_Q, [_S, _P, _P, _Q]),
    "wpt_host_lookat": (None, [_P] * 4),
    "wpt_host_generate_mesh": (_U, [_I, _I, _I, _F, _P, _P, _U, C.POINTER(_U)]),
    "wpt_host_image_load": (_Q, [_S, _P, _P, _Q]),
    "wpt_host_image_save": (_I, [_S, _U, _U, _U, _U, _P]),
    "wpt_host_mcpt": (_I, [_SCENE, _U, _U, _U, _F, _F, _P, _U]),
    "wpt_host_get_ground_truth": (_I, [_SCENE, _U, _U, _P, _P, _P, _P]),
    "wpt_host_postproc": (_I, [_I, _U, _U, _U, _P, _P, _F, _F]),
    # no wrapper below: the tests call these through lib() (tests/test_oracle_golden.py, tests/test_import.py)
    "wpt_host_transformation": (None, [_P, _F, _P, _P, _P, _P]),
    "wpt_host_transformation_chains": (None, [_P]),
    "wpt_host_projection": (None, [_F, _F, _P]),
    "wpt_host_animation_at": (None, [_P, _U, _I, _P, _P]),
    "wpt_host_compute_normals": (None, [_U, _P, _U, _P, _I, _P]),
    "wpt_host_compute_tangents": (None, [_U, _P, _P, _P, _U, _P, _P]),
    "wpt_host_obj_dump": (_I, [_S, _S]),
}


def lib():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        try:
            # the HIP runtime this process uses must be one: PyTorch ships its own libamdhip64, and when the system's copy
            # gets loaded first (this library links it) the two runtimes do not both see the device
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, (restype, argtypes) in FUNCTIONS.items():
            fn = getattr(L, name, None)  # (WPT_LIB_DIR may name an older build, which lacks the newer names)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def default_params():
    """Parameters() of the reference (wurblpt.hpp:89-95) plus the default SensorRGB gates."""
    p = _abi.Params()
    lib().wpt_host_default_params(C.byref(p))
    return p


def shutter(row_time, from_top=True):
    """The record of a rolling shutter for DeviceScene.render_shutter: one row is read every `row_time` (rounded to float32),
    from the top row down or from the bottom row up.  Row r is then exposed over device.shutter_row_interval(...) in the place
    of [t0, t1]; a scene with moving triangles must be bounded for device.shutter_span(...)."""
    s = _abi.Shutter()
    s.row_time, s.from_top = float(row_time), 1 if from_top else 0
    return s


class HostScene:
    """A built and flattened scene with its camera; owns the host buffers."""

    def __init__(self, handle, width, height, name):
        if not handle:
            raise RuntimeError("scene construction failed: %s" % name)
        self._handle = handle
        self.width, self.height, self.name = width, height, name
        self.desc = lib().wpt_host_scene_desc(handle)
        self.camera = lib().wpt_host_scene_camera(handle)
        self._handle_for_camera = handle
        self.bvh_levels = lib().wpt_host_scene_bvh_levels(handle)

    def __del__(self):
        if getattr(self, "_handle", None):
            try:
                lib().wpt_host_scene_free(self._handle)
            except TypeError:   # interpreter shutdown: the module globals are gone already
                pass
            self._handle = None

    @property
    def d(self):
        return self.desc.contents

    def set_envmap_tables(self, M, Ms, Mcs):
        """Attaches importance tables (numpy arrays, kept alive here) to the scene description;
        without them wpt_scene_upload builds them on the device."""
        self._env_tables = (M, Ms, Mcs)
        e = self.d.envmap
        e.M, e.Ms, e.Mcs = M.ctypes.data, Ms.ctypes.data, Mcs.ctypes.data

    def nodes_array(self):
        n = self.d.node_count
        return np.ctypeslib.as_array(C.cast(self.d.nodes, C.POINTER(C.c_uint32)), shape=(n, 8)).copy()


def set_distortion(scene, model, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0):
    """Lens distortion for the scene's camera: model 1 RadialAndPlanar(k1,k2,p1,p2), 2 RadialOnly(k1,k2,k3),
    3 OpenCV(k1,k2,k3,p1,p2), 0 none."""
    lib().wpt_host_scene_set_distortion(scene._handle_for_camera, model, k1, k2, k3, p1, p2)


def set_camera_mode(scene, surround_mode=0, stereoscopic_distance=0.0):
    """Camera::surroundMode (0 off, 1 = 180 degrees, 2 = 360 degrees) and ::stereoscopicDistance."""
    lib().wpt_host_scene_set_camera_mode(scene._handle_for_camera, surround_mode, stereoscopic_distance)


def lookat(eye, target, up=(0.0, 1.0, 0.0)):
    """Transformation::fromLookAt(eye, target, up) as wpt_host_lookat gives it: 35 float32 -- translation (3), rotation
    quaternion x y z w (4), scaling (3), then toMat4 (16) and toNormalMatrix (9)."""
    e, t, u = (np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(3)) for x in (eye, target, up))
    out = np.zeros(35, dtype=np.float32)
    lib().wpt_host_lookat(C.c_void_p(e.ctypes.data), C.c_void_p(t.ctypes.data), C.c_void_p(u.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def camera_looking_at(scene, eye, target, up=(0.0, 1.0, 0.0)):
    """A copy of the scene's camera (frustum, lens, distortion, mode, animation) placed at `eye` looking at `target`: its
    translation, rotation and scaling are those of lookat(eye, target, up).  For DeviceScene.render_views."""
    cam = _abi.Camera.from_buffer_copy(scene.camera.contents)
    T = lookat(eye, target, up)
    cam.translation[:] = [float(x) for x in T[0:3]]
    cam.rotation[:] = [float(x) for x in T[3:7]]
    cam.scaling[:] = [float(x) for x in T[7:10]]
    return cam


def lens_camera(frustum, model=0, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0):
    """The camera record (_abi.Camera) of a lens on a projection, for the image operations of device.py (lens_warp,
    distance_to_coords), which read nothing else of it: `frustum` = (l, r, b, t) of Projection at distance 1, `model` and the
    coefficients as in set_distortion.  dist_center, dist_focal_length and dist_inverse_focal_length are Projection::center(),
    focalLength() and inverseFocalLength() and b1 .. b4 the RadialOnly model's inverse series, in float32 with the reference's
    order of operations (optics.hpp:86-99, 170-173).  All-zero coefficients mean no distortion, as there."""
    f = np.float32
    l, r, b, t = (f(x) for x in frustum)
    k1, k2, k3, p1, p2 = (f(x) for x in (k1, k2, k3, p1, p2))
    if model not in (0, 1, 2, 3):
        raise ValueError("lens_camera: model 0 (none), 1 (RadialAndPlanar), 2 (RadialOnly) or 3 (OpenCV)")
    if model == 1:
        k3 = f(0)
    elif model == 2:
        p1 = p2 = f(0)
    elif model == 0:
        k1 = k2 = k3 = p1 = p2 = f(0)
    cam = _abi.Camera()
    cam.l, cam.r, cam.b, cam.t = l, r, b, t
    cam.rotation[3] = 1.0
    cam.scaling[:] = [1.0, 1.0, 1.0]
    cam.focus_dist = 1.0
    cam.animation = -1
    cam.distortion_type = model if any(float(x) != 0.0 for x in (k1, k2, k3, p1, p2)) else 0
    cam.k1, cam.k2, cam.k3, cam.p1, cam.p2 = k1, k2, k3, p1, p2
    if model == 2:
        cam.b1 = -k1
        cam.b2 = f(3) * k1 * k1 - k2
        cam.b3 = f(-12) * k1 * k1 * k1 + f(8) * k1 * k2 - k3
        cam.b4 = f(55) * k1 * k1 * k1 * k1 - f(55) * k1 * k1 * k2 + f(5) * k2 * k2 + f(10) * k1 * k3
    cam.dist_center[:] = [l / (l - r), b / (b - t)]
    cam.dist_focal_length[:] = [f(1) / (r - l), f(1) / (t - b)]
    cam.dist_inverse_focal_length[:] = [r - l, t - b]
    return cam


def cornell(width, height, tall_box_material=0, short_object_material=0):
    """Cornell box of wurblpt-cornellbox.cpp: tall box 0 = white / 1 = GGX metal,
    short box 0 = white / 2 = glass / 3 = glass with a refractive index per channel (chromatic dispersion: the channels'
    optical path lengths differ)."""
    h = lib().wpt_host_cornell(tall_box_material, 0, short_object_material, width, height)
    return HostScene(h, width, height, "cornell(tall=%d,short=%d)" % (tall_box_material, short_object_material))


def cornell_checker(width, height):
    """The Cornell box (GGX tall box, glass short box) whose walls, floor and ceiling carry checker textures of their colour and a
    quarter of it: a small textured scene, for what a denoiser does to a texture."""
    return HostScene(lib().wpt_host_cornell_checker(width, height), width, height, "cornell_checker")


SPEED_OF_LIGHT = 299792458.0  # m/s in vacuum (the reference's constants.hpp)


def tof_sensor(phase_image_count=4, modulation_frequency=10e6, exposure_time=1000.0, pixel_area=12.0 * 12.0, contrast=0.75):
    """The record of a SensorTofAmcw with the reference's defaults (sensor_tof_amcw.hpp:75-88) for DeviceScene.render_tof:
    frac_modfreq_c = float32(modulation_frequency / c), the division made in double; tau_j = j * (2.0f * pi) / count in the
    reference's float order.  exposure_time in microseconds, pixel_area in square micrometers."""
    if not 1 <= phase_image_count <= _abi.TOF_MAX_PHASES:
        raise ValueError("tof_sensor: 1 .. %d phase images" % _abi.TOF_MAX_PHASES)
    s = _abi.TofSensor()
    s.pixel_area, s.exposure_time, s.contrast = pixel_area, exposure_time, contrast
    s.frac_modfreq_c = float(np.float32(float(modulation_frequency) / SPEED_OF_LIGHT))
    s.phase_count = phase_image_count
    two_pi = np.float32(2.0) * np.float32(np.pi)
    for j in range(phase_image_count):
        s.tau[j] = float(np.float32(j) * two_pi / np.float32(phase_image_count))
    return s


def tof_scene(width, height, variant=0, twin=0, t0=0.0, t1=0.0):
    """Scenes for the time-of-flight sensor, camera at the origin looking along -z with a vertical field of view of 70 degrees.
    variant 0: the room of wurblpt-tof-example at rest at time 0 (wall, ModPhong quad and icosahedron, a two-sided ToF light
    at the camera); 1: the same room with its animations, bounded for the exposure interval [t0, t1] (pass the same t0, t1 in
    the render parameters); 2: a wall, a two-sided ToF light at the camera and a Cornell-class box (small enough for LDS);
    3: a glass slab of thickness 0.5 and index (1.5, 1.5, 1.5, 1.3), no dispersion, between the camera and a ToF light that
    faces it; 4: the room's wall and light alone; 5: a ToF light with an emission texture facing the camera and a cube it lights.
    twin 1 replaces LightTof(r, angle) by LightSpot(angle, vec3(r)): under SensorRGB its x channel is the ToF scene's fourth;
    twin 2 by LightSpot(angle, vec3(0)): what an RGB sensor sees of the ToF scene."""
    return HostScene(lib().wpt_host_tof_scene(variant, twin, t0, t1, width, height), width, height, "tof_scene(variant=%d,twin=%d)" % (variant, twin))


def random_triangles(n, seed, width, height, with_texcoords=True, aperture=0.0):
    h = lib().wpt_host_random_triangles(n, seed, 1 if with_texcoords else 0, width, height, aperture)
    return HostScene(h, width, height, "random_triangles(%d,%d)" % (n, seed))


def lds_edge_scene(triangles, materials, light=0, seed=1, width=40, height=32):
    """A lit, closed room with seeded clutter for the capacity edges of the kernels that keep the scene in LDS: tri_count is
    exactly `triangles` (>= 14: 12 of the room, 2 of the ceiling light, the rest clutter with edges 0.2 to 0.6 of the room's),
    node_count 2 * triangles - 1 and material_count exactly `materials`.  light 0: a LightDiffuse, one record; 1: a LightSpot
    and 2: a LightTof, each the front side of a MaterialTwoSided with a black back side -- three records (front, back, then the
    wrapper, which is the record the light's triangles name), all counted in `materials`.  The K = materials - 1 (or - 3)
    records in front of the light's are the surfaces': Lambertians of pairwise different colours, with K >= 3 record K - 2 a
    GGX and K - 3 a glass record.  Clutter triangle c has record K - 1 - c % K and the room's quads go on from there, so the
    highest records are the ones in use and, where there are more records than surfaces, the low ones belong to no triangle.
    Lights 1 and 2 make twins: the same geometry and records but for the light's front side."""
    h = lib().wpt_host_lds_edge_scene(triangles, materials, light, seed, width, height)
    return HostScene(h, width, height, "lds_edge_scene(%d,%d,light=%d,seed=%d)" % (triangles, materials, light, seed))


def sponza_like(width, height, seed=1, detail=1.0, tex_size=1024, env_width=2048, importance_n=512):
    """BASELINE config 3 stand-in: seeded Sponza-class courtyard (about 262 k triangles at
    detail 1.0), textured Lambertian / ModPhong / two-sided / GGX / mirror materials, normal
    maps, procedural sun + sky environment map with importance sampling."""
    h = lib().wpt_host_sponza_like(seed, detail, tex_size, env_width, importance_n, width, height)
    return HostScene(h, width, height, "sponza_like(seed=%d,detail=%g)" % (seed, detail))


def animated(width, height, variant=0, t0=0.0, t1=1.0):
    """A room with a turning cube, a swinging panel, a sliding light and a moving camera, bounded for the exposure
    interval [t0, t1] (pass the same t0, t1 in the render parameters).  variant bit 0: thin lens; bit 1: static
    camera; bit 2: static instances."""
    return HostScene(lib().wpt_host_animated(variant, t0, t1, width, height), width, height, "animated(variant=%d)" % variant)


def courtyard_like(width, height, seed=2, triangles=10_000_000, tex_size=1024):
    """BASELINE config 4 stand-in: seeded San-Miguel-class courtyard dominated by foliage (clouds
    of small two-sided leaf quads), every material two-sided, constant environment without
    importance sampling (wurblpt-san-miguel.cpp:36-44).  `triangles` is the approximate total."""
    h = lib().wpt_host_courtyard_like(seed, triangles, tex_size, width, height)
    return HostScene(h, width, height, "courtyard_like(seed=%d,triangles=%d)" % (seed, triangles))


def furnace(width, height, material=0, slices=64):
    """wurblpt-furnace-test.cpp with a tessellated sphere: one material in a constant environment
    of radiance 1.  material: 0 Lambertian 0.42, 1 Lambertian 1, 2 ModPhong(1,0), 3 ModPhong(0,1),
    4 ModPhong(.5,.5), 5 GGX albedo 1 roughness 0.5; on an analytic sphere: 6 clear glass (no absorption, index 1.5),
    7 perfect mirror."""
    h = lib().wpt_host_furnace(material, slices, width, height)
    return HostScene(h, width, height, "furnace(material=%d)" % material)


def mis_test(width, height, with_hot_spots=True, light_mask=15):
    """The scene of wurblpt-mis-test.cpp: four GGX plates under four sphere lights in a white room; the lights are hot
    spots (next-event estimation with MIS) or not (material sampling alone).  light_mask: bit i = light i exists."""
    h = lib().wpt_host_mis_test(1 if with_hot_spots else 0, light_mask, width, height)
    return HostScene(h, width, height, "mis_test(hot_spots=%d,lights=%d)" % (with_hot_spots, light_mask))


def texture_probe(width, height, compat=0):
    """A textured quad light in front of a float environment map, for checking what a camera ray sees directly
    (wpt_host_texture_probe); compat 0 = Mitsuba, 1 = surround video orientation of the environment."""
    return HostScene(lib().wpt_host_texture_probe(compat, width, height), width, height, "texture_probe(compat=%d)" % compat)


def spheres(width, height, variant=0):
    """Scenes with analytic spheres (HitableSphere): 0 = textured / GGX / glass / mirror spheres lit by
    a sphere light and a quad light (both hot spots), 1 = the same under a cube environment map,
    2 = wurblpt-furnace-test.cpp as written (every sphere pixel is exactly 0.42), 3 = inside a large
    emitting sphere that is a hot spot."""
    h = lib().wpt_host_spheres(variant, width, height)
    return HostScene(h, width, height, "spheres(variant=%d)" % variant)


def spot_scene(width, height, variant=0):
    """Scenes lit by LightSpots: 0 = the Cornell box (white boxes) with the spot ceiling light of wurblpt-cornellbox.cpp
    (MaterialTwoSided(LightSpot(radians(30), vec3(4)), MaterialLambertian(vec3(0)))), 1 = a stage (floor, back wall, a
    sphere) under coloured spots, one with a checker-textured emission and one a sphere, 2 = the Cornell box with GGX tall
    box, glass short box and the spot ceiling light."""
    return HostScene(lib().wpt_host_spot_scene(variant, width, height), width, height, "spot_scene(variant=%d)" % variant)


def light_groups_scene(width, height, variant=0, t0=0.0, t1=0.0, dispersive=False):
    """Scenes with several emitters for the light-groups launch (DeviceScene.render_light_groups).  0 = a closed box of
    Lambertian walls with a GGX and a glass cube under two diffuse ceiling lamps of different colour, both hot spots (small
    enough for the kernels that keep the scene in LDS); 1 = variant 0's room and lamps plus a two-sided spot lamp, a ModPhong
    panel whose emission has a checker texture, a sphere lamp that is a hot spot, and an equirect environment without
    importance tables (N = 0) seen through the open front; 2 = two lamps, one of them moving on key frames, over a swinging
    panel, bounded for the exposure interval [t0, t1] (pass the same t0, t1 in the render parameters); 3 = two lamps over two
    plates with the measured BRDFs of the committed fixtures (rgl_fixture).  dispersive (variant 0 only): the glass cube has a
    refractive index per channel, so the channels' optical path lengths differ."""
    h = lib().wpt_host_light_groups_scene(variant | (16 if dispersive else 0), t0, t1, rgl_fixture("iso").encode(),
                                          rgl_fixture("aniso").encode(), width, height)
    return HostScene(h, width, height, "light_groups_scene(variant=%d)" % variant)


def _emission(m):
    """the four floats of a material record that scale its emission, or None for a record that never emits"""
    if m.type in (_abi.MAT_LIGHT_DIFFUSE, _abi.MAT_LIGHT_SPOT):
        return m.v[0]
    if m.type == _abi.MAT_MODPHONG:
        return m.v[3]
    return None


def emitters(scene):
    """The indices of the scene's material records that emit: LIGHT_DIFFUSE, LIGHT_SPOT and MODPHONG records whose emission
    factor (v[0], v[3]) is not all zero, and MODPHONG records with an emission texture (tex[4], which stands in the factor's
    place).  A two-sided material's record is not one; its children are."""
    d = scene.d
    out = []
    for i in range(d.material_count):
        m = d.materials[i]
        e = _emission(m)
        if e is not None and (any(float(x) != 0.0 for x in e) or (m.type == _abi.MAT_MODPHONG and m.tex[4] >= 0)):
            out.append(i)
    return out


def mute_emitters(scene, keep):
    """Zeroes IN PLACE the emission factor of every emitting material record whose index is not in `keep`: the muted twin of the
    scene for the group `keep`.  A MODPHONG record's emission texture stands in its factor's place, so the record lets go of it
    (tex[4] = -1) and emits the zeroed factor.  Texture records stay as they are.  The environment is not a material; it stays
    too (mute_environment)."""
    keep = set(int(k) for k in keep)
    d = scene.d
    for i in emitters(scene):
        if i not in keep:
            m = d.materials[i]
            e = _emission(m)
            for c in range(4):
                e[c] = 0.0
            if m.type == _abi.MAT_MODPHONG:
                m.tex[4] = -1
    return scene


def mute_environment(scene):
    """Zeroes IN PLACE the value factor and offset of the environment map's textures (a constant's or a checker's colours): the
    environment of a muted twin.  Only where that changes no table: a scene with hot spots never samples the environment by
    importance, and one with N = 0 has no tables; anything else raises ValueError."""
    d = scene.d
    e = d.envmap
    if e.type == 0:
        return scene
    if e.N > 0 and d.hotspot_count == 0:
        raise ValueError("mute_environment: the environment's importance tables would change")
    for t in ([e.tex] if e.type == 1 else list(e.cube_tex)):
        tex = d.textures[t]  # (a transformer's own factor and offset: its child may belong to a material as well)
        for c in range(4):
            tex.a[c] = 0.0
            tex.b[c] = 0.0
    return scene


def rgl_fixture(name):
    """path of a synthetic measured-BRDF file committed under tests/golden (iso / aniso)"""
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "synthetic_%s.bsdf" % name)


def rgl_build(filename):
    """The model's tables for a BRDF file, as MaterialRGL builds them: (_abi.RglBrdf, float32 pool)."""
    n = lib().wpt_host_rgl_build(filename.encode(), None, None, 0)
    if n == 0:
        raise RuntimeError("cannot read %s as a measured BRDF" % filename)
    brdf = _abi.RglBrdf()
    pool = np.zeros(n, np.float32)
    lib().wpt_host_rgl_build(filename.encode(), C.byref(brdf), C.c_void_p(pool.ctypes.data), n)
    return brdf, pool


def rgl_scene(width, height, variant=0, file0=None, file1=None):
    """Scenes with MaterialRGL: 0 = furnace test, 1 = two measured spheres under a quad light."""
    f0 = file0 or rgl_fixture("iso")
    f1 = file1 or rgl_fixture("aniso")
    h = lib().wpt_host_rgl_scene(variant, f0.encode(), f1.encode(), width, height)
    return HostScene(h, width, height, "rgl_scene(variant=%d)" % variant)


def measured_like(width, height, rgl0, rgl1, seed=3, detail=1.0, tex_size=1024, env_width=2048, importance_n=512):
    """BASELINE config 5 stand-in: the Sponza-class architecture with measured BRDFs (MaterialRGL, two
    tensor files) and normal maps on walls, columns, beams and vases; environment importance sampling."""
    h = lib().wpt_host_measured_like(seed, detail, tex_size, env_width, importance_n, rgl0.encode(), rgl1.encode(), width, height)
    return HostScene(h, width, height, "measured_like(seed=%d,detail=%g)" % (seed, detail))


IMPORT_DISABLE_LIGHT_SOURCES, IMPORT_DISABLE_HOT_SPOTS, IMPORT_TWO_SIDED_MATERIALS, IMPORT_INVERTED_TF, IMPORT_WITH_GLASS = 1, 2, 4, 8, 16


def import_obj(filename, width, height, eye, at, vfov_degrees=45.0, import_bits=0, scale=1.0, rotate_y_degrees=0.0, env_radiance=0.0):
    """importIntoScene (include/wurblpt/import.hpp) of an OBJ file, an optional constant environment and a
    look-at camera; None if the file cannot be imported."""
    e = (C.c_float * 3)(*eye)
    a = (C.c_float * 3)(*at)
    h = lib().wpt_host_import_obj(filename.encode(), import_bits, scale, rotate_y_degrees, env_radiance, e, a, vfov_degrees, width, height)
    return HostScene(h, width, height, "import_obj(%s)" % os.path.basename(filename)) if h else None


def import_obj_env(filename, envmap, width, height, eye, at, vfov_degrees=45.0, import_bits=0, scale=1.0, rotate_y_degrees=0.0, importance_n=0):
    """importIntoScene of an OBJ file under an environment map read from an image file, as wurblpt-sponza.cpp:46-59 sets
    its scene up; importance_n > 0: initializeImportanceSampling(importance_n).  None if a file cannot be read."""
    e = (C.c_float * 3)(*eye)
    a = (C.c_float * 3)(*at)
    h = lib().wpt_host_import_obj_env(filename.encode(), envmap.encode(), importance_n, import_bits, scale, rotate_y_degrees, e, a, vfov_degrees, width, height)
    return HostScene(h, width, height, "import_obj_env(%s, %s)" % (os.path.basename(filename), os.path.basename(envmap))) if h else None


def image_load(filename):
    """Decodes an image file with the importer's decoders: numpy array [h, w, comps], row 0 = bottom."""
    info = (C.c_uint * 4)()
    n = lib().wpt_host_image_load(filename.encode(), info, None, 0)
    if n == 0:
        return None
    dtype = [np.uint8, np.uint16, np.float32][info[3]]
    out = np.zeros((info[1], info[0], info[2]), dtype=dtype)
    lib().wpt_host_image_load(filename.encode(), info, C.c_void_p(out.ctypes.data), n)
    return out


def mcpt(scene, samples_sqrt, t0=0.0, t1=0.0, width=None, height=None, workers=1):
    """mcpt() of include/wurblpt/wurblpt.hpp (needs a device): the scene, its camera and a SensorRGB through the C++
    host API an application uses; returns the frame [h, w, 3]."""
    w = width or scene.width
    h = height or scene.height
    frame = np.zeros((h, w, 3), np.float32)
    if not lib().wpt_host_mcpt(scene._handle, w, h, samples_sqrt, t0, t1, C.c_void_p(frame.ctypes.data), workers):
        raise RuntimeError("mcpt failed")
    return frame


def scene_tag(scene):
    """sceneTag() of include/wurblpt/progressive.hpp: the 64-bit fingerprint of a flattened scene that a saved progressive
    session carries and DeviceScene.resume compares -- FNV-1a over the description's arrays (nodes, tri_geom, tri_attr, instances,
    materials, textures, texels, hotspots, spheres, rgl_brdfs, rgl_data, animations, keyframes; each as its length in bytes, 8
    bytes little endian, then its bytes) and the environment map's type, compat, tex, N and cube_tex.  Computed by the C++
    function itself, so the two sides cannot drift apart."""
    return int(lib().wpt_host_scene_tag(scene.desc))


MESH_KINDS = {"quad": 0, "cube": 1, "cube_side": 2, "disk": 3, "sphere": 4, "cylinder": 5, "closed_cylinder": 6, "cone": 7,
              "closed_cone": 8, "torus": 9, "tetrahedron": 10, "octahedron": 11, "icosahedron": 12}


def generate_mesh(kind, a=1, b=1, f=0.0):
    """A mesh of include/wurblpt/generator.hpp: (vertices float32 [n, 11] = position, normal, texcoord, tangent; indices
    uint32 [triangles, 3])."""
    cap = 1 << 16
    v = np.zeros((cap, 11), np.float32)
    ind = np.zeros(3 * cap, np.uint32)
    ni = C.c_uint(0)
    n = lib().wpt_host_generate_mesh(MESH_KINDS[kind], a, b, f, C.c_void_p(v.ctypes.data), C.c_void_p(ind.ctypes.data), cap, C.byref(ni))
    assert n <= cap and ni.value <= 3 * cap
    return v[:n].copy(), ind[:ni.value].reshape(-1, 3).copy()


def material_scene_index(scene):
    """Scene::materialIndex() of every flattened material (what getGroundTruth reports for it)."""
    out = np.zeros(scene.d.material_count, np.int32)
    lib().wpt_host_scene_material_scene_index(scene._handle, C.c_void_p(out.ctypes.data))
    return out


def get_ground_truth(scene, bits=(1 << 20) - 1, prev_from_at=None, next_from_at=None, width=None, height=None, times=None):
    """getGroundTruth() of include/wurblpt/wurblpt.hpp (needs a device) for the scene's look-at camera without
    lens; prev_from_at / next_from_at: 6 floats, eye and target of the camera at tPrev / tNext."""
    from . import device
    w = width or scene.width
    h = height or scene.height
    arrays, ptrs = device.gt_arrays(w, h, bits)
    tm = (C.c_float * 3)(*times) if times is not None else None
    pf = np.ascontiguousarray(prev_from_at, np.float32) if prev_from_at is not None else None
    nf = np.ascontiguousarray(next_from_at, np.float32) if next_from_at is not None else None
    if not lib().wpt_host_get_ground_truth(scene._handle, w, h, C.c_void_p(pf.ctypes.data) if pf is not None else None,
                                           C.c_void_p(nf.ctypes.data) if nf is not None else None, tm, ptrs):
        raise RuntimeError("getGroundTruth failed")
    return {device.GT_NAMES[k]: a for k, a in enumerate(arrays) if a is not None}


def image_save(filename, img):
    """Writes a numpy image [h, w, comps] (uint8, uint16 or float32; row 0 = bottom) by file name extension."""
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    code = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}[img.dtype]
    return bool(lib().wpt_host_image_save(filename.encode(), img.shape[1], img.shape[0], img.shape[2], code,
                                          C.c_void_p(img.ctypes.data)))


def postproc(op, img, a=0.0, b=0.0):
    """The output side through include/wurblpt/postproc.hpp (needs a device): "srgb" -> toSRGB, "urq" ->
    uniformRationalQuantization(a=maxVal, b=brightness), "scale" -> scaleLuminance(a=factor, b=clamp),
    "maxlum" -> maxLuminance.  img: float32 [h, w, comps >= 3]."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    code = {"srgb": 0, "urq": 1, "scale": 2, "maxlum": 3}[op]
    out = (np.zeros(img.shape[:2] + (3,), np.uint8) if code == 0 else
           np.zeros(1, np.float32) if code == 3 else np.zeros(img.shape, np.float32))
    if not lib().wpt_host_postproc(code, img.shape[1], img.shape[0], img.shape[2], C.c_void_p(img.ctypes.data),
                                   C.c_void_p(out.ctypes.data), a, b):
        raise RuntimeError("post-processing failed")
    return float(out[0]) if code == 3 else out


def bvh_build(boxes):
    """boxes: float32 [n, 6] (lo, hi) -> (uint32 [nodes, 8] raw node words, levels)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    n = boxes.shape[0]
    out = np.zeros((max(2 * n - 1, 1), 8), dtype=np.uint32)
    levels = C.c_uint(0)
    cnt = lib().wpt_host_bvh_build(n, boxes.ctypes.data, out.ctypes.data, C.byref(levels))
    return out[:cnt], levels.value
