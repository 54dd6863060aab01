"""The first-hit colour pass and the demodulated denoiser on the GPU: the pass's guide arrays are the ground truth pass's bits; its
emission plane is what the CPU restatement's path tracer adds for the first hit; its albedo plane is the emission plane of a twin
scene whose surfaces are lamps of their own colour; wpt_postproc_denoise_demodulated gives the bits of its host twin; a frame
rendered, described and filtered without leaving the device equals the host twin fed with the downloaded arrays.  What the
demodulated filter does to the error against a converged render is measured, not asserted: on the scenes measured it gains
nothing over the plain filter (profiles/denoise_demodulated_quality.txt, tools/denoise_demodulated_quality.py)."""
import numpy as np
import pytest

from tests import denoise_cases as cases
from tests import oracle_loader
from wurblpt_amd import _abi, host

pytestmark = pytest.mark.gpu

AROUND_A_TILE = ((31, 15), (32, 16), (33, 17), (31, 17), (65, 15))      # tests/test_gpu_denoise.py's
SMALL_SPONZA = dict(detail=0.05, tex_size=32, env_width=64, importance_n=16)
LIGHTS = (_abi.MAT_LIGHT_DIFFUSE, _abi.MAT_LIGHT_SPOT)
COLOURED = (_abi.MAT_LAMBERTIAN, _abi.MAT_GGX, _abi.MAT_MIRROR, _abi.MAT_MODPHONG)

@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from wurblpt_amd import device
    return device


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def positive_zero(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def params_at(t0=0.0):
    p = host.default_params()
    p.randomize_ray_over_pixel = 0
    p.t0 = p.t1 = t0
    return p


GUIDE_SCENES = {
    "cornell_lambertian": (lambda: host.cornell(33, 9), 0.0),
    "cornell_ggx_glass": (lambda: host.cornell(64, 64, tall_box_material=1, short_object_material=2), 0.0),
    "cornell_dispersive_glass": (lambda: host.cornell(40, 32, tall_box_material=0, short_object_material=3), 0.0),
    "spot_stage": (lambda: host.spot_scene(40, 32, 1), 0.0),
    "spot_cornell": (lambda: host.spot_scene(33, 9, 0), 0.0),
    "spheres": (lambda: host.spheres(32, 24, 0), 0.0),
    "spheres_cube_environment": (lambda: host.spheres(40, 32, 1), 0.0),
    "animated": (lambda: host.animated(40, 32, 0, 0.0, 1.0), 0.375),
    "texture_probe": (lambda: host.texture_probe(32, 24), 0.0),
    "lds_edge": (lambda: host.lds_edge_scene(64, 4), 0.0),
    "sponza_small": (lambda: host.sponza_like(40, 32, **SMALL_SPONZA), 0.0),
}


@pytest.mark.parametrize("name", sorted(GUIDE_SCENES))
def test_guide_arrays_are_the_ground_truth_passes(dev, name):
    import torch
    make, t0 = GUIDE_SCENES[name]
    sc = make()
    if name == "texture_probe":
        host.set_distortion(sc, 3, k1=-0.1, k2=0.02, p1=0.01)          # the lens distortion is followed as it is there
    ds = dev.DeviceScene(sc)
    p = params_at(t0)
    want = ds.ground_truth_device(params=p, times=(t0, t0, t0))
    got = ds.first_hit_colours_device(params=p)
    alone = ds.first_hit_colours_device(albedo=False, emission=False, params=p)      # the guide without the colours
    colours = ds.first_hit_colours_device(guide=False, params=p)                     # and the colours without the guide
    torch.cuda.synchronize()
    ds.check()
    assert sorted(got) == sorted(dev.GUIDE_NAMES + ("albedo", "emission")) and sorted(alone) == sorted(dev.GUIDE_NAMES)
    for k in dev.GUIDE_NAMES:
        assert got[k].dtype == want[k].dtype and bits_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), (name, k)
        assert bits_equal(alone[k].cpu().numpy(), want[k].cpu().numpy()), (name, k)
    for k in ("albedo", "emission"):
        assert bits_equal(colours[k].cpu().numpy(), got[k].cpu().numpy()) and np.isfinite(got[k].cpu().numpy()).all()
    m = want["materials"].cpu().numpy()
    assert (m >= 0).any() and len(np.unique(m)) >= 2
    # the numpy form is the same launch
    arrays = dev.first_hit_colours(ds, params=p)
    for k in got:
        assert bits_equal(arrays[k], got[k].cpu().numpy()), (name, k)
    ds.close()


def black(rec):
    return rec.type == _abi.MAT_LAMBERTIAN and rec.tex[0] < 0 and not any(float(x) != 0.0 for x in list(rec.v[0])[:3])


def pixel_classes(sc, materials):
    """per pixel, from the first hit's record m (two-sided wrappers looked through as far as both sides agree):
    'lamp'      what the path tracer adds for the first hit is all the frame holds: nothing hit; a light; a wrapper whose front is
                a light and whose back is a light too or a black Lambertian without a texture (the frame's back side is 0 * ...)
    'coloured'  one of the four kinds with an albedo, or a wrapper of two of them
    'one'       glass, a measured BRDF seen from its front
    'dark'      everything whose albedo is +0 by the rule: nothing hit, lights, a wrapper of a light and a black Lambertian"""
    d = sc.d
    kind = {-1: ("lamp", "dark")}
    for m in range(d.material_count):
        rec = d.materials[m]
        if rec.type in LIGHTS:
            kind[m] = ("lamp", "dark")
        elif rec.type in COLOURED:
            kind[m] = ("surface", "coloured")
        elif rec.type in (_abi.MAT_GLASS, _abi.MAT_RGL):
            kind[m] = ("surface", "one")
        elif rec.type == _abi.MAT_TWOSIDED:
            front, back = d.materials[rec.tex[0]], d.materials[rec.tex[1]]
            if front.type in LIGHTS and (back.type in LIGHTS or black(back)):
                kind[m] = ("lamp", "dark")
            elif front.type in COLOURED and back.type in COLOURED:
                kind[m] = ("surface", "coloured")
            else:
                kind[m] = ("other", "other")
        else:
            kind[m] = ("surface", "dark")
    flat = materials.reshape(-1)
    lamp = np.array([kind[int(m)][0] == "lamp" for m in flat]).reshape(materials.shape[:2])
    surface = np.array([kind[int(m)][0] == "surface" for m in flat]).reshape(materials.shape[:2])
    albedo = np.array([kind[int(m)][1] for m in flat]).reshape(materials.shape[:2])
    return lamp, surface, albedo


EMISSION_SCENES = {
    "texture_probe_mitsuba": lambda: host.texture_probe(32, 24, 0),
    "texture_probe_surround": lambda: host.texture_probe(33, 9, 1),
    "spheres_cube_environment": lambda: host.spheres(40, 32, 1),
    "inside_an_emitting_sphere": lambda: host.spheres(32, 24, 3),
    "spot_stage": lambda: host.spot_scene(40, 32, 1),
    "spot_cornell": lambda: host.spot_scene(40, 32, 0),
    "measured_spheres_under_an_environment": lambda: host.rgl_scene(40, 32, 1),
}


@pytest.mark.parametrize("name", sorted(EMISSION_SCENES))
def test_emission_is_what_the_path_tracer_adds_for_the_first_hit(dev, name):
    """The CPU restatement's frame at one sample per pixel through the pixel's centre, pinhole: tracePath adds 1.0f * emitted for
    the first hit and a light scatters nothing, a miss adds 1.0f * envL -- so on the 'lamp' pixels (pixel_classes) the frame IS
    the emission, bit for bit.  Every other compared pixel lies on a surface that does not emit (none of these scenes has an
    emissive ModPhong): +0."""
    import torch
    sc = EMISSION_SCENES[name]()
    sc.camera.contents.lens_radius = 0.0
    p = params_at()
    assert not [i for i in host.emitters(sc) if sc.d.materials[i].type == _abi.MAT_MODPHONG]
    frame, _ = oracle_loader.load("portable").render(sc, 1, params=p)
    ds = dev.DeviceScene(sc)
    got = ds.first_hit_colours_device(params=p)
    torch.cuda.synchronize()
    ds.check()
    emission, materials = got["emission"].cpu().numpy(), got["materials"].cpu().numpy()
    ds.close()
    lamp, surface, _ = pixel_classes(sc, materials)
    print("%s: %d of %d pixels see a lamp or nothing, %d of them lit; %d a surface" % (name, lamp.sum(), lamp.size, emission[lamp].any(axis=1).sum(), surface.sum()))
    assert lamp.sum() * 10 >= lamp.size
    if name.startswith("texture_probe"):
        assert lamp.all()
    assert bits_equal(emission[lamp], frame[lamp])
    assert positive_zero(emission[surface])
    assert name == "spot_cornell" or emission[lamp].any()             # (that camera sees the lamp's rim at most: nothing hit, no environment)


def twin_of(sc):
    """IN PLACE: every record with an albedo becomes a diffuse light of that colour -- the same tex[0], and v[0] = 1 where the
    texture gives the colour.  A diffuse light emits v[0] * texel on its front and 0 on its back."""
    d = sc.d
    for m in range(d.material_count):
        rec = d.materials[m]
        if rec.type in COLOURED:
            rec.type = _abi.MAT_LIGHT_DIFFUSE
            if rec.tex[0] >= 0:
                for c in range(4):
                    rec.v[0][c] = 1.0
    return sc


ALBEDO_SCENES = {
    "cornell_ggx_glass": lambda: host.cornell(64, 64, tall_box_material=1, short_object_material=2),
    "sponza_small": lambda: host.sponza_like(40, 32, **SMALL_SPONZA),
    "checker_cornell": lambda: host.cornell_checker(40, 32),
    "measured_spheres": lambda: host.rgl_scene(32, 24, 1),
}


@pytest.mark.parametrize("name", sorted(ALBEDO_SCENES))
def test_albedo_is_the_emission_of_the_twin_whose_surfaces_are_lamps(dev, name):
    import torch
    p = params_at()
    sc = ALBEDO_SCENES[name]()
    ds = dev.DeviceScene(sc)
    got = ds.first_hit_colours_device(params=p)
    torch.cuda.synchronize()
    ds.check()
    albedo, materials = got["albedo"].cpu().numpy(), got["materials"].cpu().numpy()
    ds.close()
    _, _, kind = pixel_classes(sc, materials)               # before the records change
    twin = dev.DeviceScene(twin_of(ALBEDO_SCENES[name]()))
    lit = twin.first_hit_colours_device(params=p)
    torch.cuda.synchronize()
    twin.check()
    twin_emission = lit["emission"].cpu().numpy()
    assert bits_equal(lit["materials"].cpu().numpy(), materials)
    twin.close()
    print("%s: %s" % (name, {k: int((kind == k).sum()) for k in np.unique(kind)}))
    coloured = kind == "coloured"
    assert coloured.sum() * 10 >= coloured.size and bits_equal(albedo[coloured], twin_emission[coloured])
    assert albedo[coloured].any() and np.isfinite(albedo).all()
    assert (albedo[kind == "one"] == 1.0).all() and positive_zero(albedo[kind == "dark"])
    if name != "sponza_small":
        assert (kind == "one").any() and (kind == "dark").any()
    if name == "checker_cornell":                           # a checker: two colours inside one record
        m = materials.reshape(materials.shape[:2])
        assert max(len(np.unique(albedo[(m == k) & coloured], axis=0)) for k in np.unique(m[coloured])) == 2
    if name == "sponza_small":                              # textures: the albedo varies inside one record
        m = materials.reshape(materials.shape[:2])
        assert max(len(np.unique(albedo[(m == k) & coloured], axis=0)) for k in np.unique(m[coloured])) > 8


def colour_planes(c, seed=5):
    """albedo channels that are 0, below the floor, the floor or anything up to 1; a tenth of the pixels emit, a quarter of them
    more than the frame holds (u < 0)"""
    h, w = c["frame"].shape[:2]
    rng = np.random.RandomState(seed * 7919 + w * 31 + h)
    floor = np.float32(_abi.DENOISE_ALBEDO_FLOOR)
    pick = rng.randint(0, 8, (h, w, 3))
    albedo = np.where(pick == 0, 0, np.where(pick == 1, floor / 2, np.where(pick == 2, floor, rng.rand(h, w, 3)))).astype(np.float32)
    emits = (rng.rand(h, w) < 0.1)[..., None]
    more = (rng.rand(h, w) < 0.25)[..., None]
    emission = np.where(emits, np.where(more, c["frame"] + rng.rand(h, w, 3), c["frame"] * rng.rand(h, w, 3)), 0).astype(np.float32)
    return albedo, emission


@pytest.mark.parametrize("kind,size", [("mixed", s) for s in cases.SIZES + AROUND_A_TILE] + [("sky", (33, 9)), ("unsampled", (130, 70))])
def test_demodulated_device_equals_host_twin(dev, kind, size):
    import torch
    w, h = size
    c = dict(cases.inputs(w, h, kind, seed=13))
    c["albedo"], c["emission"] = colour_planes(c)
    names = ("frame", "moments", "samples_sqrt", "positions", "normals", "materials", "albedo", "emission")
    on_device = {k: torch.from_numpy(c[k].view(np.int16) if k == "samples_sqrt" else c[k]).cuda() for k in names}
    on_device["samples_sqrt"] = on_device["samples_sqrt"].view(torch.uint16)
    before = {k: t.clone() for k, t in on_device.items()}
    guide = (on_device["positions"], on_device["normals"], on_device["materials"])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for iterations in range(9):
        p = _abi.DenoiseParams(iterations=iterations)
        got, var = dev.denoise_demodulated(on_device["frame"], on_device["moments"], on_device["samples_sqrt"], guide, on_device["albedo"],
                                           on_device["emission"], p, variance_out=True, stream=stream)
        alone = dev.denoise_demodulated(on_device["frame"], on_device["moments"], on_device["samples_sqrt"], guide, on_device["albedo"],
                                        on_device["emission"], p, stream=stream)
        stream.synchronize()
        want, want_var = dev.denoise_demodulated_host(c["frame"], c["moments"], c["samples_sqrt"], cases.guide(c), c["albedo"], c["emission"], p,
                                                      variance_out=True)
        assert bits_equal(got.cpu().numpy(), want) and bits_equal(var.cpu().numpy(), want_var), (kind, size, iterations)
        assert bits_equal(alone.cpu().numpy(), want)
        assert np.isfinite(want).all() and np.isfinite(want_var).all()
    for k in names:
        assert torch.equal(on_device[k].view(torch.int16) if k == "samples_sqrt" else on_device[k],
                           before[k].view(torch.int16) if k == "samples_sqrt" else before[k]), k
    # a floor of its own, and one number for a constant map
    other = dev.denoise_demodulated(on_device["frame"], on_device["moments"], 2, guide, on_device["albedo"], on_device["emission"], albedo_floor=0.25)
    torch.cuda.synchronize()
    assert bits_equal(other.cpu().numpy(), dev.denoise_demodulated_host(c["frame"], c["moments"], 2, cases.guide(c), c["albedo"], c["emission"],
                                                                        albedo_floor=0.25))


@pytest.fixture(scope="module")
def textured(dev):
    """the small Sponza-class scene 64 x 64: the 16-spp frame with its moment film, the first-hit colours with the guide and both
    filtered frames, all on the device"""
    import torch
    ds = dev.DeviceScene(host.sponza_like(64, 64, **SMALL_SPONZA))
    m = np.full((64, 64), 4, np.uint16)
    frame, moments = ds.render_adaptive(m, with_moments=True)
    colours = ds.first_hit_colours_device()
    demodulated, variance = dev.denoise_demodulated(frame, moments, m, colours, variance_out=True)
    plain = dev.denoise(frame, moments, m, colours)
    torch.cuda.synchronize()
    ds.check()
    ds.close()
    return {"map": m, "frame": frame, "moments": moments, "colours": colours, "demodulated": demodulated, "variance": variance, "plain": plain}


def test_rendered_described_and_filtered_on_the_device(dev, textured):
    colours = {k: v.cpu().numpy() for k, v in textured["colours"].items()}
    frame, moments = textured["frame"].cpu().numpy(), textured["moments"].cpu().numpy()
    want, want_var = dev.denoise_demodulated_host(frame, moments, textured["map"], colours, variance_out=True)
    assert bits_equal(textured["demodulated"].cpu().numpy(), want) and bits_equal(textured["variance"].cpu().numpy(), want_var)
    assert bits_equal(textured["plain"].cpu().numpy(), dev.denoise_host(frame, moments, textured["map"], colours))
    assert not bits_equal(want, textured["plain"].cpu().numpy()) and np.isfinite(want).all()


def test_the_example_runs(tmp_path):
    """examples/denoise_textured.cpp through getFirstHitColours() and both overloads of denoise(), at 48 x 32: three pictures"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "wurblpt_amd", "lib")
    exe = str(tmp_path / "denoise_textured")
    subprocess.run(["g++", "-std=c++20", "-O1", "-fopenmp", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "denoise_textured.cpp"),
                    "-L" + lib, "-lwurblpt_hip", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, "48", "32", "2", "3", str(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
    pictures = [open(str(tmp_path / name), "rb").read() for name in ("textured-noisy.png", "textured-denoised.png", "textured-demodulated.png")]
    assert min(len(p) for p in pictures) > 100 and len(set(pictures)) == 3      # three different pictures
