"""The scenes of host.lds_edge_scene that sit on the capacity edges of the kernels with the scene in LDS, shared by
tests/test_lds_edge_scenes.py (CPU: each scene is on its side of its edge and its surfaces show) and tests/test_gpu_lds_edges.py
(the frames).  The sizes are picked from the byte equations of DESIGN.md section 4, "Sizes on the edges of the LDS layout"; what a
launch is expected to do is never taken from them but from wpt_kernel_choice for the scene's own counts, and `side()` then says
in words which side of every edge that is, so that a change to the layout fails the tests loudly instead of moving them off
their edges."""
import functools

from wurblpt_amd import _abi, device, host

WG = 256                       # lanes of a workgroup: the stride of the loops that copy the scene into LDS
TWOSIDED, GGX, GLASS, SPOT, ROTATED = 16, 32, 64, 2048, 16384      # feature bits (wpt_device.h)
LDS_MATERIALS, LDS_FOLD = 1, 2
W, H, S = 40, 32, 2            # the frames: 40 x 32 at samples_sqrt 2

# the seed of each size: with it the oracle's frame is lit in more than half its pixels and the tree has the folded links that
# test_lds_edge_scenes.py states, for every number of materials and every light the size is used with (the clutter is the
# same for all of them; the order of the triangles, and with it of equal boxes in the tree's build, is not)
SEED = {16: 9, 32: 2, 36: 2, 37: 2, 64: 2, 65: 2, 85: 10, 86: 10, 183: 18, 184: 18}

# Plain frames, materials behind the rotated copies: (triangles, materials) -> the side the default walk must be on
PLAIN = {
    (16, 34): "rotated, materials in LDS in 2 trips",      # 40 960 bytes: exact fill; 272 quadwords of material records
    (16, 35): "rotated, materials in HBM",
    (32, 8): "rotated, materials in LDS in 1 trip",        # 40 960 bytes: exact fill
    (32, 9): "rotated, materials in HBM",
    (36, 2): "rotated, materials in HBM",                  # 40 768 bytes: the last size whose copies fit
    (37, 2): "select, materials in LDS in 1 trip",         # 40 976 bytes with the copies
}
# Every kernel that does not rotate, one scene per edge: (triangles, materials) -> the side of a launch that selects the corners
SENSORS = {
    (16, 34): "select, materials in LDS in 2 trips",       # (not an edge of its own: the one size whose material loop goes round twice)
    (32, 32): "select, materials in LDS in 1 trip",        # 40 960 bytes: exact fill; 256 quadwords, the last lane's
    (32, 33): "select, materials in HBM",
    (64, 2): "select, materials in LDS in 1 trip",         # nodes: 254 quadwords
    (65, 2): "select, materials in LDS in 1 trip",         # nodes: 258
    (85, 2): "select, materials in HBM",                   # corners: 255
    (86, 2): "select, materials in HBM",                   # corners: 258
    (183, 2): "select, materials in HBM",                  # 20 464 bytes of scene, a request of 53 776
    (184, 2): "HBM",                                       # 20 576 bytes of scene
}
# The time-of-flight kernel: light 2, whose MaterialTwoSided takes three records where a LightDiffuse takes one.  The same total
# keeps the edges of the material records; a scene of two records becomes one of four (one surface record, as before), and the
# edges of the node and corner loops stay where they are
TOF = {
    (16, 34): "select, materials in LDS in 2 trips",
    (32, 32): "select, materials in LDS in 1 trip",
    (32, 33): "select, materials in HBM",
    (64, 4): "select, materials in LDS in 1 trip",         # 40 960 bytes with its four records
    (65, 4): "select, materials in HBM",
    (85, 4): "select, materials in HBM",
    (86, 4): "select, materials in HBM",
    (183, 4): "select, materials in HBM",
    (184, 4): "HBM",
}
# trips of the node and the corner loops, (nodes, corners), where a scene is in LDS
TRIPS = {16: (1, 1), 32: (1, 1), 36: (1, 1), 37: (1, 1), 64: (1, 1), 65: (2, 1), 85: (2, 1), 86: (2, 2), 183: (3, 3)}


@functools.lru_cache(maxsize=None)
def scene(triangles, materials, light=0, width=W, height=H):
    return host.lds_edge_scene(triangles, materials, light, SEED[triangles], width, height)


def need(sc):
    """the feature bits the library finds in the scene's material records (sceneFeatures, wpt_capi_scene.hip)"""
    bits = {_abi.MAT_TWOSIDED: TWOSIDED, _abi.MAT_GGX: GGX, _abi.MAT_GLASS: GLASS, _abi.MAT_LIGHT_SPOT: SPOT}
    types = {sc.d.materials[i].type for i in range(sc.d.material_count)}
    assert types <= set(bits) | {_abi.MAT_LAMBERTIAN, _abi.MAT_LIGHT_DIFFUSE}
    return sum(bits.get(t, 0) for t in types)


def choice(sc, sensor, walk=0, variant=0):
    """wpt_kernel_choice for the scene's own counts: (name, form, key, sceneLdsBytes, materialsInLds)"""
    d = sc.d
    return device.kernel_choice(need(sc), sensor, False, d.node_count, d.tri_count, d.material_count, False, variant, walk)


def trips(quadwords):
    return -(-quadwords // WG)


def side(sc, chosen):
    """the side of every edge a choice is on, in the words of PLAIN and SENSORS"""
    _, form, key, lds_bytes, word = chosen
    if not key[2]:
        assert lds_bytes == 0
        return "HBM"
    assert (form == "rotated corners") == bool(key[0] & ROTATED)
    d = sc.d
    copies = 3 if key[0] & ROTATED else 1
    scene_bytes = 32 * d.node_count + 32 + 48 * copies * d.tri_count
    if word & LDS_MATERIALS:
        assert lds_bytes == scene_bytes + 128 * d.material_count
        where = "LDS in %d trip%s" % (trips(8 * d.material_count), "s" if trips(8 * d.material_count) > 1 else "")
    else:
        assert lds_bytes == scene_bytes
        where = "HBM"
    return "%s, materials in %s" % ("rotated" if key[0] & ROTATED else "select", where)


def loop_trips(sc):
    """trips of the loops that copy the nodes and the corners"""
    return trips(2 * sc.d.node_count), trips(3 * sc.d.tri_count)


def folded_nodes(sc):
    """indices of the nodes whose word in LDS is not their first child: the links the fold takes out start there"""
    folded, words = device.fold_plan(sc, with_words=True)
    return folded, [i for i in range(sc.d.node_count) if words[i] < 2 ** 31 and words[i] != i + 1]
