"""wpt_kernel_choice: which instantiation of wpt_pathtrace renders a launch, as a pure host function (no device).  The expected
rows are written out by hand from the table of rules in DESIGN.md section 4, "Which kernel renders a launch"; nothing here
restates the rules in code."""
import os

import pytest

from wurblpt_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# feature bits (wpt_device.h)
TEXTURES, ENVMAP, TWOSIDED, GGX, GLASS, RGL, ANIM, TRANSIENT, SPOT, VIEWS, ADAPTIVE, ROTATED, TOF, SLICED = (
    1, 4, 16, 32, 64, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
BASIC = 96      # FEAT_GGX | FEAT_GLASS
ALL = 2303      # textures, modified Phong, environment, lens, two-sided, GGX, glass, spheres, spot lights
WALK_SELECT_CORNERS, WALK_NO_FOLD = 16, 32
LDS_MATERIALS, LDS_FOLD = 1, 2
SENSORS = {"frame": 0, "transient": 1, "views": 2, "adaptive": 3, "tof": 4}

# every instantiation but the two sliced twins: (F, COUNT, LDSSCENE, WIDE), wpt_kernel_name
KERNELS = {
    "lds": ((BASIC, False, True, False), "wpt_pathtrace"),
    "lds_rot": ((BASIC | ROTATED, False, True, False), "wpt_pathtrace"),
    "basic": ((BASIC, False, False, False), "wpt_pathtrace"),
    "basic_count": ((BASIC, True, False, False), "wpt_pathtrace"),
    "full": ((ALL, False, False, False), "wpt_pathtrace"),
    "full_wide": ((ALL, False, False, True), "wpt_pathtrace, wide walk"),
    "full_count": ((ALL, True, False, False), "wpt_pathtrace"),
    "rgl": ((ALL | RGL, False, False, False), "wpt_pathtrace"),
    "rgl_wide": ((ALL | RGL, False, False, True), "wpt_pathtrace, wide walk"),
    "rgl_count": ((ALL | RGL, True, False, False), "wpt_pathtrace"),
    "anim": ((ALL | ANIM, False, False, False), "wpt_pathtrace"),
    "anim_count": ((ALL | ANIM, True, False, False), "wpt_pathtrace"),
    "rgl_anim": ((ALL | RGL | ANIM, False, False, False), "wpt_pathtrace"),
    "rgl_anim_count": ((ALL | RGL | ANIM, True, False, False), "wpt_pathtrace"),
    "tr_lds": ((BASIC | TRANSIENT, False, True, False), "wpt_pathtrace, transient, scene in LDS"),
    "tr_full": ((ALL | TRANSIENT, False, False, False), "wpt_pathtrace, transient, all features"),
    "tr_anim": ((ALL | ANIM | TRANSIENT, False, False, False), "wpt_pathtrace, transient, all features, moving scenes"),
    "tr_rgl": ((ALL | RGL | ANIM | TRANSIENT, False, False, False), "wpt_pathtrace, transient, measured BRDFs"),
    "tof_lds": ((BASIC | TWOSIDED | SPOT | TOF, False, True, False), "wpt_pathtrace, time of flight, scene in LDS"),
    "tof_full": ((ALL | TOF, False, False, False), "wpt_pathtrace, time of flight, all features"),
    "tof_anim": ((ALL | ANIM | TOF, False, False, False), "wpt_pathtrace, time of flight, all features, moving scenes"),
    "tof_rgl": ((ALL | RGL | ANIM | TOF, False, False, False), "wpt_pathtrace, time of flight, measured BRDFs"),
    "views_lds": ((BASIC | VIEWS, False, True, False), "wpt_pathtrace, views, scene in LDS"),
    "views_basic": ((BASIC | VIEWS, False, False, False), "wpt_pathtrace, views, basic"),
    "views_basic_count": ((BASIC | VIEWS, True, False, False), "wpt_pathtrace, views, basic, counting"),
    "views_full": ((ALL | VIEWS, False, False, False), "wpt_pathtrace, views, all features"),
    "views_full_count": ((ALL | VIEWS, True, False, False), "wpt_pathtrace, views, all features, counting"),
    "views_anim": ((ALL | ANIM | VIEWS, False, False, False), "wpt_pathtrace, views, all features, moving scenes"),
    "views_anim_count": ((ALL | ANIM | VIEWS, True, False, False), "wpt_pathtrace, views, all features, moving scenes, counting"),
    "views_rgl": ((ALL | RGL | ANIM | VIEWS, False, False, False), "wpt_pathtrace, views, measured BRDFs"),
    "views_rgl_count": ((ALL | RGL | ANIM | VIEWS, True, False, False), "wpt_pathtrace, views, measured BRDFs, counting"),
    "ad_lds": ((BASIC | ADAPTIVE, False, True, False), "wpt_pathtrace, adaptive, scene in LDS"),
    "ad_basic": ((BASIC | ADAPTIVE, False, False, False), "wpt_pathtrace, adaptive, basic"),
    "ad_full": ((ALL | ADAPTIVE, False, False, False), "wpt_pathtrace, adaptive, all features"),
    "ad_anim": ((ALL | ANIM | ADAPTIVE, False, False, False), "wpt_pathtrace, adaptive, all features, moving scenes"),
    "ad_rgl": ((ALL | RGL | ANIM | ADAPTIVE, False, False, False), "wpt_pathtrace, adaptive, measured BRDFs"),
}
SLICED_TWINS = [(BASIC | SLICED, False, True, False), (BASIC | ROTATED | SLICED, False, True, False)]

# the strings of the name ladders renderLaunch had before the table, and wpt_kernel_name's default
NAMES_BEFORE_THE_TABLE = {
    "wpt_pathtrace", "wpt_pathtrace, wide walk",
    "wpt_pathtrace, transient, scene in LDS", "wpt_pathtrace, transient, measured BRDFs",
    "wpt_pathtrace, transient, all features, moving scenes", "wpt_pathtrace, transient, all features",
    "wpt_pathtrace, views, scene in LDS", "wpt_pathtrace, views, measured BRDFs, counting", "wpt_pathtrace, views, measured BRDFs",
    "wpt_pathtrace, views, all features, moving scenes, counting", "wpt_pathtrace, views, all features, moving scenes",
    "wpt_pathtrace, views, basic, counting", "wpt_pathtrace, views, basic",
    "wpt_pathtrace, views, all features, counting", "wpt_pathtrace, views, all features",
    "wpt_pathtrace, adaptive, scene in LDS", "wpt_pathtrace, adaptive, measured BRDFs",
    "wpt_pathtrace, adaptive, all features, moving scenes", "wpt_pathtrace, adaptive, basic", "wpt_pathtrace, adaptive, all features",
    "wpt_pathtrace, time of flight, scene in LDS", "wpt_pathtrace, time of flight, measured BRDFs",
    "wpt_pathtrace, time of flight, all features, moving scenes", "wpt_pathtrace, time of flight, all features",
}

# Scene classes: feature bits, nodes, triangles, materials.  The Cornell box is 71 nodes, 36 triangles and 6 materials of 128
# bytes: 71 * 32 + 32 + 36 * 48 = 4032 bytes in LDS, 7488 with two more copies of the corners, which with the 33 280 bytes of
# the paths' own words is 40 768 of the 40 960 a workgroup may use -- so the rotated form fits, and its 768 bytes of material
# records then do not, while behind the plain copy they do (4800).
SCENES = {
    "cornell": (GGX | GLASS, 71, 36, 6),
    "big": (GGX | GLASS, 1999, 1000, 6),                                    # basic, 111 968 bytes: over the 20 480 of a scene in LDS
    "textured": (TEXTURES | ENVMAP | TWOSIDED | GGX, 19999, 10000, 30),
    "rgl": (GGX | RGL, 23, 12, 3),                                          # measured BRDFs; small enough for LDS, which has no such kernel
    "tofbasic": (GGX | GLASS | SPOT | TWOSIDED, 71, 36, 6),                 # the Cornell box lit by a two-sided spot light
}
# materialsInLds of a launch that is not rotated (the records fit behind every scene that fits, and the tree is folded), and
# the bytes the kernels with the scene in LDS ask for
WORD = {"cornell": LDS_MATERIALS | LDS_FOLD, "big": LDS_FOLD, "textured": LDS_FOLD, "rgl": LDS_MATERIALS | LDS_FOLD, "tofbasic": LDS_MATERIALS | LDS_FOLD}
LDS_BYTES = {"lds": 4800, "lds_rot": 7488, "tr_lds": 4800, "tof_lds": 4800, "views_lds": 4800, "ad_lds": 4800}

# default flags: sensor, scene, anim, count, wide form uploaded -> kernel
DEFAULT_ROWS = [
    ("frame", "cornell", 0, 0, 0, "lds_rot"),
    ("frame", "cornell", 0, 0, 1, "lds_rot"),
    ("frame", "cornell", 0, 1, 0, "basic_count"),
    ("frame", "cornell", 0, 1, 1, "basic_count"),
    ("frame", "cornell", 1, 0, 0, "anim"),
    ("frame", "cornell", 1, 0, 1, "anim"),
    ("frame", "cornell", 1, 1, 0, "anim_count"),
    ("frame", "cornell", 1, 1, 1, "anim_count"),
    ("frame", "big", 0, 0, 0, "basic"),
    ("frame", "big", 0, 0, 1, "full_wide"),
    ("frame", "big", 0, 1, 0, "basic_count"),
    ("frame", "big", 0, 1, 1, "basic_count"),
    ("frame", "big", 1, 0, 0, "anim"),
    ("frame", "big", 1, 0, 1, "anim"),
    ("frame", "big", 1, 1, 0, "anim_count"),
    ("frame", "big", 1, 1, 1, "anim_count"),
    ("frame", "textured", 0, 0, 0, "full"),
    ("frame", "textured", 0, 0, 1, "full_wide"),
    ("frame", "textured", 0, 1, 0, "full_count"),
    ("frame", "textured", 0, 1, 1, "full_count"),
    ("frame", "textured", 1, 0, 0, "anim"),
    ("frame", "textured", 1, 0, 1, "anim"),
    ("frame", "textured", 1, 1, 0, "anim_count"),
    ("frame", "textured", 1, 1, 1, "anim_count"),
    ("frame", "rgl", 0, 0, 0, "rgl"),
    ("frame", "rgl", 0, 0, 1, "rgl_wide"),
    ("frame", "rgl", 0, 1, 0, "rgl_count"),
    ("frame", "rgl", 0, 1, 1, "rgl_count"),
    ("frame", "rgl", 1, 0, 0, "rgl_anim"),
    ("frame", "rgl", 1, 0, 1, "rgl_anim"),
    ("frame", "rgl", 1, 1, 0, "rgl_anim_count"),
    ("frame", "rgl", 1, 1, 1, "rgl_anim_count"),
    ("frame", "tofbasic", 0, 0, 0, "full"),
    ("frame", "tofbasic", 0, 0, 1, "full_wide"),
    ("frame", "tofbasic", 0, 1, 0, "full_count"),
    ("frame", "tofbasic", 0, 1, 1, "full_count"),
    ("frame", "tofbasic", 1, 0, 0, "anim"),
    ("frame", "tofbasic", 1, 0, 1, "anim"),
    ("frame", "tofbasic", 1, 1, 0, "anim_count"),
    ("frame", "tofbasic", 1, 1, 1, "anim_count"),
    ("transient", "cornell", 0, 0, 0, "tr_lds"),
    ("transient", "cornell", 0, 0, 1, "tr_lds"),
    ("transient", "cornell", 1, 0, 0, "tr_anim"),
    ("transient", "cornell", 1, 0, 1, "tr_anim"),
    ("transient", "big", 0, 0, 0, "tr_full"),
    ("transient", "big", 0, 0, 1, "tr_full"),
    ("transient", "big", 1, 0, 0, "tr_anim"),
    ("transient", "big", 1, 0, 1, "tr_anim"),
    ("transient", "textured", 0, 0, 0, "tr_full"),
    ("transient", "textured", 0, 0, 1, "tr_full"),
    ("transient", "textured", 1, 0, 0, "tr_anim"),
    ("transient", "textured", 1, 0, 1, "tr_anim"),
    ("transient", "rgl", 0, 0, 0, "tr_rgl"),
    ("transient", "rgl", 0, 0, 1, "tr_rgl"),
    ("transient", "rgl", 1, 0, 0, "tr_rgl"),
    ("transient", "rgl", 1, 0, 1, "tr_rgl"),
    ("transient", "tofbasic", 0, 0, 0, "tr_full"),
    ("transient", "tofbasic", 0, 0, 1, "tr_full"),
    ("transient", "tofbasic", 1, 0, 0, "tr_anim"),
    ("transient", "tofbasic", 1, 0, 1, "tr_anim"),
    ("views", "cornell", 0, 0, 0, "views_lds"),
    ("views", "cornell", 0, 0, 1, "views_lds"),
    ("views", "cornell", 0, 1, 0, "views_basic_count"),
    ("views", "cornell", 0, 1, 1, "views_basic_count"),
    ("views", "cornell", 1, 0, 0, "views_anim"),
    ("views", "cornell", 1, 0, 1, "views_anim"),
    ("views", "cornell", 1, 1, 0, "views_anim_count"),
    ("views", "cornell", 1, 1, 1, "views_anim_count"),
    ("views", "big", 0, 0, 0, "views_basic"),
    ("views", "big", 0, 0, 1, "views_basic"),
    ("views", "big", 0, 1, 0, "views_basic_count"),
    ("views", "big", 0, 1, 1, "views_basic_count"),
    ("views", "big", 1, 0, 0, "views_anim"),
    ("views", "big", 1, 0, 1, "views_anim"),
    ("views", "big", 1, 1, 0, "views_anim_count"),
    ("views", "big", 1, 1, 1, "views_anim_count"),
    ("views", "textured", 0, 0, 0, "views_full"),
    ("views", "textured", 0, 0, 1, "views_full"),
    ("views", "textured", 0, 1, 0, "views_full_count"),
    ("views", "textured", 0, 1, 1, "views_full_count"),
    ("views", "textured", 1, 0, 0, "views_anim"),
    ("views", "textured", 1, 0, 1, "views_anim"),
    ("views", "textured", 1, 1, 0, "views_anim_count"),
    ("views", "textured", 1, 1, 1, "views_anim_count"),
    ("views", "rgl", 0, 0, 0, "views_rgl"),
    ("views", "rgl", 0, 0, 1, "views_rgl"),
    ("views", "rgl", 0, 1, 0, "views_rgl_count"),
    ("views", "rgl", 0, 1, 1, "views_rgl_count"),
    ("views", "rgl", 1, 0, 0, "views_rgl"),
    ("views", "rgl", 1, 0, 1, "views_rgl"),
    ("views", "rgl", 1, 1, 0, "views_rgl_count"),
    ("views", "rgl", 1, 1, 1, "views_rgl_count"),
    ("views", "tofbasic", 0, 0, 0, "views_full"),
    ("views", "tofbasic", 0, 0, 1, "views_full"),
    ("views", "tofbasic", 0, 1, 0, "views_full_count"),
    ("views", "tofbasic", 0, 1, 1, "views_full_count"),
    ("views", "tofbasic", 1, 0, 0, "views_anim"),
    ("views", "tofbasic", 1, 0, 1, "views_anim"),
    ("views", "tofbasic", 1, 1, 0, "views_anim_count"),
    ("views", "tofbasic", 1, 1, 1, "views_anim_count"),
    ("adaptive", "cornell", 0, 0, 0, "ad_lds"),
    ("adaptive", "cornell", 0, 0, 1, "ad_lds"),
    ("adaptive", "cornell", 1, 0, 0, "ad_anim"),
    ("adaptive", "cornell", 1, 0, 1, "ad_anim"),
    ("adaptive", "big", 0, 0, 0, "ad_basic"),
    ("adaptive", "big", 0, 0, 1, "ad_basic"),
    ("adaptive", "big", 1, 0, 0, "ad_anim"),
    ("adaptive", "big", 1, 0, 1, "ad_anim"),
    ("adaptive", "textured", 0, 0, 0, "ad_full"),
    ("adaptive", "textured", 0, 0, 1, "ad_full"),
    ("adaptive", "textured", 1, 0, 0, "ad_anim"),
    ("adaptive", "textured", 1, 0, 1, "ad_anim"),
    ("adaptive", "rgl", 0, 0, 0, "ad_rgl"),
    ("adaptive", "rgl", 0, 0, 1, "ad_rgl"),
    ("adaptive", "rgl", 1, 0, 0, "ad_rgl"),
    ("adaptive", "rgl", 1, 0, 1, "ad_rgl"),
    ("adaptive", "tofbasic", 0, 0, 0, "ad_full"),
    ("adaptive", "tofbasic", 0, 0, 1, "ad_full"),
    ("adaptive", "tofbasic", 1, 0, 0, "ad_anim"),
    ("adaptive", "tofbasic", 1, 0, 1, "ad_anim"),
    ("tof", "cornell", 0, 0, 0, "tof_lds"),
    ("tof", "cornell", 0, 0, 1, "tof_lds"),
    ("tof", "cornell", 1, 0, 0, "tof_anim"),
    ("tof", "cornell", 1, 0, 1, "tof_anim"),
    ("tof", "big", 0, 0, 0, "tof_full"),
    ("tof", "big", 0, 0, 1, "tof_full"),
    ("tof", "big", 1, 0, 0, "tof_anim"),
    ("tof", "big", 1, 0, 1, "tof_anim"),
    ("tof", "textured", 0, 0, 0, "tof_full"),
    ("tof", "textured", 0, 0, 1, "tof_full"),
    ("tof", "textured", 1, 0, 0, "tof_anim"),
    ("tof", "textured", 1, 0, 1, "tof_anim"),
    ("tof", "rgl", 0, 0, 0, "tof_rgl"),
    ("tof", "rgl", 0, 0, 1, "tof_rgl"),
    ("tof", "rgl", 1, 0, 0, "tof_rgl"),
    ("tof", "rgl", 1, 0, 1, "tof_rgl"),
    ("tof", "tofbasic", 0, 0, 0, "tof_lds"),
    ("tof", "tofbasic", 0, 0, 1, "tof_lds"),
    ("tof", "tofbasic", 1, 0, 0, "tof_anim"),
    ("tof", "tofbasic", 1, 0, 1, "tof_anim"),
]

# one override at a time: sensor, (need, nodes, triangles, materials), anim, count, wide, variant, walk
#   -> kernel, form, sceneLdsBytes, materialsInLds
CORNELL = SCENES["cornell"]
OVERRIDE_ROWS = [
    # variant 1: the scene stays in HBM
    ("frame", CORNELL, 0, 0, 0, 1, 0, "basic", "", 0, 3),
    ("frame", CORNELL, 0, 0, 1, 1, 0, "full_wide", "", 0, 3),
    ("transient", CORNELL, 0, 0, 0, 1, 0, "tr_full", "", 0, 3),
    ("views", CORNELL, 0, 0, 0, 1, 0, "views_basic", "", 0, 3),
    ("adaptive", CORNELL, 0, 0, 0, 1, 0, "ad_basic", "", 0, 3),
    ("tof", SCENES["tofbasic"], 0, 0, 0, 1, 0, "tof_full", "", 0, 3),
    # variant 2: all features
    ("frame", CORNELL, 0, 0, 0, 2, 0, "full", "", 0, 3),
    ("frame", CORNELL, 0, 1, 0, 2, 0, "full_count", "", 0, 3),
    ("transient", CORNELL, 0, 0, 0, 2, 0, "tr_full", "", 0, 3),
    ("views", CORNELL, 0, 0, 0, 2, 0, "views_full", "", 0, 3),
    ("views", CORNELL, 0, 1, 0, 2, 0, "views_full_count", "", 0, 3),
    ("adaptive", CORNELL, 0, 0, 0, 2, 0, "ad_full", "", 0, 3),
    ("tof", CORNELL, 0, 0, 0, 2, 0, "tof_full", "", 0, 3),
    # WPT_WALK_SELECT_CORNERS: the kernel that selects, and the material records behind its one copy
    ("frame", CORNELL, 0, 0, 0, 0, WALK_SELECT_CORNERS, "lds", "", 4800, 3),
    ("transient", CORNELL, 0, 0, 0, 0, WALK_SELECT_CORNERS, "tr_lds", "", 4800, 3),
    # WPT_WALK_NO_FOLD
    ("frame", CORNELL, 0, 0, 0, 0, WALK_NO_FOLD, "lds_rot", "rotated corners", 7488, 0),
    ("transient", CORNELL, 0, 0, 0, 0, WALK_NO_FOLD, "tr_lds", "", 4800, 1),
    ("frame", SCENES["big"], 0, 0, 0, 0, WALK_NO_FOLD, "basic", "", 0, 0),
    # variant 0x80: the material records stay in HBM
    ("adaptive", CORNELL, 0, 0, 0, 0x80, 0, "ad_lds", "", 4032, 2),
    ("frame", CORNELL, 0, 0, 0, 0x80, WALK_SELECT_CORNERS, "lds", "", 4032, 2),
    ("frame", (GGX | GLASS, 71, 36, 1), 0, 0, 0, 0x80, 0, "lds_rot", "rotated corners", 7488, 2),
    # the rotated copies fit: one material record behind them fills 40 896 of 40 960 bytes, two would need 41 024
    ("frame", (GGX | GLASS, 71, 36, 1), 0, 0, 0, 0, 0, "lds_rot", "rotated corners", 7616, 3),
    ("frame", (GGX | GLASS, 71, 36, 2), 0, 0, 0, 0, 0, "lds_rot", "rotated corners", 7488, 2),
    # the rotated limit: 71 * 32 + 32 + 37 * 144 = 7632 of the 7680 bytes behind the paths' words; one triangle more is 7776
    ("frame", (GGX | GLASS, 71, 37, 6), 0, 0, 0, 0, 0, "lds_rot", "rotated corners", 7632, 2),
    ("frame", (GGX | GLASS, 71, 38, 6), 0, 0, 0, 0, 0, "lds", "", 71 * 32 + 32 + 38 * 48 + 6 * 128, 3),
    # the limit of a scene in LDS: 160 * 32 + 320 * 48 = 20 480 bytes; its copy leaves no room for material records
    ("transient", (GGX | GLASS, 160, 320, 6), 0, 0, 0, 0, 0, "tr_lds", "", 20512, 2),
    ("transient", (GGX | GLASS, 160, 321, 6), 0, 0, 0, 0, 0, "tr_full", "", 0, 2),
]


def choose(sensor, scene, anim, count, wide, variant=0, walk=0):
    need, nodes, tris, materials = scene
    return device.kernel_choice(need | (ANIM if anim else 0), SENSORS[sensor], count, nodes, tris, materials, wide, variant, walk)


def test_default_rows_cover_the_cross_product():
    seen = {r[:5] for r in DEFAULT_ROWS}
    assert len(seen) == len(DEFAULT_ROWS) == 140
    for sensor in SENSORS:
        for scene in SCENES:
            for anim in (0, 1):
                for count in ((0, 1) if sensor in ("frame", "views") else (0,)):
                    for wide in (0, 1):
                        assert (sensor, scene, anim, count, wide) in seen


@pytest.mark.parametrize("sensor", sorted(SENSORS))
def test_choice_at_default_flags(sensor):
    for row in DEFAULT_ROWS:
        if row[0] != sensor:
            continue
        _, scene, anim, count, wide, kernel = row
        key, kernel_name = KERNELS[kernel]
        name, form, got_key, lds_bytes, word = choose(sensor, SCENES[scene], anim, count, wide)
        assert got_key == key, (row, got_key)
        assert name == kernel_name, (row, name)
        assert form == ("rotated corners" if kernel == "lds_rot" else ""), (row, form)
        assert lds_bytes == LDS_BYTES.get(kernel, 0), (row, lds_bytes)
        assert word == (LDS_FOLD if kernel == "lds_rot" else WORD[scene]), (row, word)


def test_choice_under_each_override():
    for row in OVERRIDE_ROWS:
        sensor, scene, anim, count, wide, variant, walk, kernel, form, lds_bytes, word = row
        key, kernel_name = KERNELS[kernel]
        assert choose(sensor, scene, anim, count, wide, variant, walk) == (kernel_name, form, key, lds_bytes, word), row


def test_rows_and_table_agree():
    table = device.kernel_table()
    keys = [k for k, _ in table]
    assert len(table) == 38 and len(set(keys)) == 38
    for kernel, (key, name) in KERNELS.items():
        assert (key, name) in table, kernel
    chosen = {KERNELS[r[5]][0] for r in DEFAULT_ROWS} | {KERNELS[r[7]][0] for r in OVERRIDE_ROWS}
    assert sorted(set(keys) - chosen) == sorted(SLICED_TWINS)
    assert {KERNELS[r[5]][1] for r in DEFAULT_ROWS} | {KERNELS[r[7]][1] for r in OVERRIDE_ROWS} == NAMES_BEFORE_THE_TABLE
    assert {name for _, name in table} == NAMES_BEFORE_THE_TABLE


def test_a_launch_without_a_kernel_is_refused_with_its_key():
    """no sensor but one frame and a batch of views has counting kernels"""
    with pytest.raises(RuntimeError, match=r"F = %d, COUNT = 1, LDSSCENE = 0, WIDE = 0.*status 4" % (ALL | TRANSIENT)):
        device.kernel_choice(GGX | TEXTURES, SENSORS["transient"], True, 71, 36, 6)
    with pytest.raises(RuntimeError, match="sensor"):
        device.kernel_choice(GGX, 5, False, 71, 36, 6)


def test_code_objects_are_recorded_unchanged():
    """profiles/kernel_table_code_objects.txt, written by tools/code_object_compare.sh: every translation unit compiles to the
    same gfx950 code object as before the table (wpt_capi among them: only its host side changed)"""
    rows = [line.split(" : ") for line in open(os.path.join(ROOT, "profiles", "kernel_table_code_objects.txt")) if not line.startswith("#")]
    verdict = {r[0]: r[-1].strip() for r in rows}
    assert len(verdict) == 45
    assert all(v == "same" for v in verdict.values()), verdict
    assert "wpt_capi" in verdict and sum(u.startswith(("wpt_k_basic", "wpt_k_full")) for u in verdict) == 37
