"""host.lds_edge_scene on the CPU: the scenes of tests/lds_edge_cases.py have the counts they are asked for, sit on the intended side
of every edge of the LDS layout (wpt_kernel_choice, no device) for each sensor tests/test_gpu_lds_edges.py renders them with, have
folded links where the fold is to be walked, and the oracle's 40 x 32 x 2^2 frame of each is lit in at least half its pixels and
shows the material records behind the 32nd.  These are conditions the seeds and the camera were picked to meet, not measurements."""
import numpy as np
import pytest

from wurblpt_amd import _abi, device

from tests import lds_edge_cases as cases

MATF_TOF_LIGHT = 16           # wurblpt_hip.h
SENSOR_NAMES = {"transient": "wpt_pathtrace, transient, scene in LDS", "views": "wpt_pathtrace, views, scene in LDS",
                "adaptive": "wpt_pathtrace, adaptive, scene in LDS", "tof": "wpt_pathtrace, time of flight, scene in LDS"}
SENSOR_IDS = {"transient": device.SENSOR_TRANSIENT, "views": device.SENSOR_VIEWS, "adaptive": device.SENSOR_ADAPTIVE,
              "tof": device.SENSOR_TOF}
ALL_SCENES = sorted({(t, m, 0) for t, m in list(cases.PLAIN) + list(cases.SENSORS)} | {(t, m, light) for t, m in cases.TOF for light in (1, 2)})


def tri_materials(sc):
    return [sc.d.tri_geom[i].material for i in range(sc.d.tri_count)]


@pytest.mark.parametrize("t,m,light", ALL_SCENES)
def test_counts_records_and_assignment(t, m, light):
    sc = cases.scene(t, m, light)
    d = sc.d
    assert (d.tri_count, d.node_count, d.material_count, d.hotspot_count, d.sphere_count) == (t, 2 * t - 1, m, 2, 0)
    records = [d.materials[i] for i in range(m)]
    k = m - (1 if light == 0 else 3)                               # the surfaces' records
    want = [_abi.MAT_LAMBERTIAN] * k
    if k >= 3:
        want[k - 2], want[k - 3] = _abi.MAT_GGX, _abi.MAT_GLASS
    want += [_abi.MAT_LIGHT_DIFFUSE] if light == 0 else [_abi.MAT_LIGHT_SPOT, _abi.MAT_LAMBERTIAN, _abi.MAT_TWOSIDED]
    assert [r.type for r in records] == want
    if light:
        assert bool(records[m - 3].flags & MATF_TOF_LIGHT) == (light == 2)
        assert (records[m - 1].tex[0], records[m - 1].tex[1]) == (m - 3, m - 2)
    colours = {tuple(r.v[0][:3]) for r in records[:k] if r.type == _abi.MAT_LAMBERTIAN}
    assert len(colours) == sum(r.type == _abi.MAT_LAMBERTIAN for r in records[:k])          # pairwise different
    # the highest records are the ones in use: the light's is the last, the surfaces use the top min(k, t - 14 + 6) of theirs
    used = set(tri_materials(sc))
    surfaces = min(k, t - 14 + 6)
    assert used == set(range(k - surfaces, k)) | {m - 1}
    assert tri_materials(sc).count(m - 1) == 2
    # clutter: edges of 0.2 to 0.6 of the room's 2, inside the room
    g = [d.tri_geom[i] for i in range(t)]
    corners = np.array([[x.v0[:], x.v1[:], x.v2[:]] for x in g], np.float64)
    assert np.abs(corners).max() == 1.0
    flat = (np.abs(corners).max(axis=1) == np.abs(corners).min(axis=1)).any(axis=1) & (np.abs(corners).max(axis=(1, 2)) >= 0.98)
    assert flat.sum() == 14                                                         # the room's walls and the light
    edges = np.linalg.norm(corners - np.roll(corners, 1, axis=1), axis=2)[~flat]
    assert edges.size == 3 * (t - 14) and (t == 14 or (edges.min() >= 0.4 and edges.max() <= 1.2))
    assert np.abs(corners[~flat]).max(initial=0.0) <= 0.97 + 1e-6


def test_sides_of_the_plain_frames():
    for (t, m), want in cases.PLAIN.items():
        sc = cases.scene(t, m)
        default = cases.choice(sc, device.SENSOR_FRAME)
        assert default[0] == "wpt_pathtrace" and cases.side(sc, default) == want, (t, m, cases.side(sc, default))
        assert default[4] & cases.LDS_FOLD
        no_fold = cases.choice(sc, device.SENSOR_FRAME, walk=device.WALK_NO_FOLD)
        assert cases.side(sc, no_fold) == want and not no_fold[4] & cases.LDS_FOLD and no_fold[2] == default[2]
        select = cases.choice(sc, device.SENSOR_FRAME, walk=device.WALK_SELECT_CORNERS)
        assert cases.side(sc, select).startswith("select, materials in LDS") and select[2] == (cases.GGX | cases.GLASS, False, True, False)
        assert cases.loop_trips(sc) == cases.TRIPS[t] == (1, 1)
    # each pair is one record, or one triangle, apart and on different sides
    assert cases.PLAIN[(16, 34)] != cases.PLAIN[(16, 35)] and cases.PLAIN[(32, 8)] != cases.PLAIN[(32, 9)] and cases.PLAIN[(36, 2)][:7] != cases.PLAIN[(37, 2)][:7]
    # the exact fills: the launch asks for every byte a workgroup may have where four share a compute unit
    cold = 40960 - cases.choice(cases.scene(16, 34), device.SENSOR_FRAME)[3]
    assert cold == 40960 - cases.choice(cases.scene(32, 8), device.SENSOR_FRAME)[3] == 33280
    assert cold + cases.choice(cases.scene(36, 2), device.SENSOR_FRAME)[3] == 40768


def test_sides_of_the_sensors_scenes():
    for (t, m), want in cases.SENSORS.items():
        sc = cases.scene(t, m)
        chosen = {"frame": cases.choice(sc, device.SENSOR_FRAME, walk=device.WALK_SELECT_CORNERS)}
        chosen.update({s: cases.choice(sc, SENSOR_IDS[s]) for s in ("transient", "views", "adaptive")})
        for sensor, c in chosen.items():
            assert cases.side(sc, c) == want, (t, m, sensor, cases.side(sc, c))
            if want != "HBM":
                assert c[0] == ("wpt_pathtrace" if sensor == "frame" else SENSOR_NAMES[sensor]) and c[1] == ""
                assert cases.loop_trips(sc) == cases.TRIPS[t]
            else:
                assert "scene in LDS" not in c[0]
    for (t, m), want in cases.TOF.items():
        sc = cases.scene(t, m, 2)
        c = cases.choice(sc, device.SENSOR_TOF)
        assert cases.side(sc, c) == want, (t, m, cases.side(sc, c))
        assert ("scene in LDS" in c[0]) == (want != "HBM") and "time of flight" in c[0]
        assert want == "HBM" or cases.loop_trips(sc) == cases.TRIPS[t]
    sides = cases.SENSORS
    assert sides[(32, 32)] != sides[(32, 33)] and sides[(183, 2)] != sides[(184, 2)]
    assert [cases.TRIPS[t] for t in (64, 65, 85, 86)] == [(1, 1), (2, 1), (2, 1), (2, 2)]
    # the exact fill, and the largest request: 33 280 bytes of the paths' own words in front of the scene's
    assert cases.choice(cases.scene(32, 32), device.SENSOR_TRANSIENT)[3] == 40960 - 33280
    assert cases.choice(cases.scene(64, 4, 2), device.SENSOR_TOF)[3] == 40960 - 33280
    assert cases.choice(cases.scene(183, 2), device.SENSOR_VIEWS)[3] + 33280 == 53776


# size -> (links the fold takes out, the nodes they start at)
FOLDS = {16: (4, [6, 7, 8, 9]), 32: (3, [20, 21, 22]), 36: (3, [26, 27, 28]), 37: (3, [26, 27, 28]), 64: (2, [1, 60]), 65: (2, [1, 62]),
         85: (4, [106, 115, 116, 140]), 86: (3, [108, 117, 142]), 183: (3, [252, 261, 262]), 184: (1, [254])}


@pytest.mark.parametrize("t", sorted(FOLDS))
def test_folded_links(t):
    """every size has folded links, and the sizes whose tree goes on far enough behind node 128 have one that starts there (of
    the 129 nodes of 65 triangles the 128th is the last leaf)"""
    m = {mm for tt, mm in list(cases.PLAIN) + list(cases.SENSORS) if tt == t}
    for sc in [cases.scene(t, mm) for mm in sorted(m)] + [cases.scene(t, mm, 2) for tt, mm in cases.TOF if tt == t]:
        assert cases.folded_nodes(sc) == FOLDS[t], sc.name
    assert FOLDS[t][0] > 0
    if t in (85, 86, 183):
        assert max(FOLDS[t][1]) >= 128


@pytest.fixture(scope="module")
def frames(oracle):
    cache = {}

    def get(t, m, light):
        if (t, m, light) not in cache:
            cache[(t, m, light)] = oracle.render(cases.scene(t, m, light), cases.S)[0]
            cache[(t, m, light)].setflags(write=False)
        return cache[(t, m, light)]
    return get


@pytest.mark.parametrize("t,m,light", ALL_SCENES)
def test_the_oracles_frame_is_lit(frames, t, m, light):
    """(a ToF light sends near infrared only: an RGB frame of it is black, and its twin with the spot light stands for it)"""
    frame = frames(t, m, 1 if light == 2 else light)
    assert frame.shape == (cases.H, cases.W, 3) and np.isfinite(frame).all()
    lit = (frame != 0).any(axis=2).mean()
    assert lit >= 0.5, lit


@pytest.mark.parametrize("t,m,light", [s for s in ALL_SCENES if s[1] > 32])
def test_records_behind_the_32nd_show(oracle, frames, t, m, light):
    """every record of index 32 or more that a triangle names changes the frame when it changes: a colour scaled, and for the
    light's MaterialTwoSided, which has none, its sides swapped"""
    sc = cases.scene(t, m, light)
    high = sorted({r for r in tri_materials(sc) if r >= 32})
    assert high and high[-1] == m - 1
    if light == 2:
        return                                                      # the twin's frame is the one to look at
    frame = frames(t, m, light)
    for r in high:
        rec = sc.d.materials[r]
        saved = _abi.Material.from_buffer_copy(rec)
        try:
            if rec.type == _abi.MAT_TWOSIDED:
                rec.tex[0], rec.tex[1] = rec.tex[1], rec.tex[0]
            else:
                for c in range(3):
                    rec.v[0][c] = 0.5 * rec.v[0][c]
            changed, _ = oracle.render(sc, cases.S)
        finally:
            sc.d.materials[r] = saved
        again, _ = oracle.render(sc, cases.S)
        assert np.array_equal(again, frame)
        differing = (changed != frame).any(axis=2).mean()
        assert differing >= 0.01, (r, differing)
