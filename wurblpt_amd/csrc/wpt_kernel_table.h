/*
 * wpt_kernel_table.h -- which instantiation of wpt_pathtrace renders a launch (host only; wpt_capi_render.hip).
 *
 * KERNEL_TABLE has one row per instantiation, findKernel looks a row up by its template arguments, and selectKernel is the
 * rule that names the row for a launch: a pure function of the facts it is given (no HIP call, nothing global), so that the
 * choice can be tested without a device (wpt_kernel_choice).  DESIGN.md section 4 has the rule as a table.
 */
#ifndef WPT_KERNEL_TABLE_H
#define WPT_KERNEL_TABLE_H

#include "wpt_pathtrace.inc.h"

namespace wptk {

struct KernelEntry {
    uint32_t features; /* F */
    bool count, ldsScene, wide;
    void (*launch)(const KernelArgs&, dim3 grid, size_t sceneLdsBytes, hipStream_t);
    const char* name; /* wpt_kernel_name: the kernel family */
};

#define WPT_KERNEL_ROW(F, COUNT, LDSSCENE, WIDE, NAME) { (F), COUNT, LDSSCENE, WIDE, launchPathtrace<(F), COUNT, LDSSCENE, WIDE>, NAME }
static const KernelEntry KERNEL_TABLE[] = {
    /* one frame: the Cornell class with the scene in LDS (select form, rotated corners, and their twins that hand pixels out in
     * slices), basic and all features from HBM, measured BRDFs; the wide walk; moving scenes; counting builds */
    WPT_KERNEL_ROW(FEAT_BASIC, false, true, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_ROTATED, false, true, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_SLICED, false, true, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_ROTATED | FEAT_SLICED, false, true, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_BASIC, false, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_BASIC, true, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL, false, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL, false, false, true, "wpt_pathtrace, wide walk"),
    WPT_KERNEL_ROW(FEAT_ALL, true, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL, false, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL, false, false, true, "wpt_pathtrace, wide walk"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL, true, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM, false, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM, true, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM, false, false, false, "wpt_pathtrace"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM, true, false, false, "wpt_pathtrace"),
    /* the transient film (args.bins): measured BRDFs take the moving-scene instantiation whether the scene moves or not, here and
     * for every sensor below */
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_TRANSIENT, false, true, false, "wpt_pathtrace, transient, scene in LDS"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_TRANSIENT, false, false, false, "wpt_pathtrace, transient, all features"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM | FEAT_TRANSIENT, false, false, false, "wpt_pathtrace, transient, all features, moving scenes"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_TRANSIENT, false, false, false, "wpt_pathtrace, transient, measured BRDFs"),
    /* the time-of-flight sensor (args.bins); its kernel with the scene in LDS knows spot lights and two-sided materials besides: a
     * ToF light has a back side */
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_TWOSIDED | FEAT_SPOT | FEAT_TOF, false, true, false, "wpt_pathtrace, time of flight, scene in LDS"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_TOF, false, false, false, "wpt_pathtrace, time of flight, all features"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM | FEAT_TOF, false, false, false, "wpt_pathtrace, time of flight, all features, moving scenes"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_TOF, false, false, false, "wpt_pathtrace, time of flight, measured BRDFs"),
    /* a batch of views (args.views): product and counting builds */
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_VIEWS, false, true, false, "wpt_pathtrace, views, scene in LDS"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_VIEWS, false, false, false, "wpt_pathtrace, views, basic"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_VIEWS, true, false, false, "wpt_pathtrace, views, basic, counting"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_VIEWS, false, false, false, "wpt_pathtrace, views, all features"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_VIEWS, true, false, false, "wpt_pathtrace, views, all features, counting"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, false, false, false, "wpt_pathtrace, views, all features, moving scenes"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM | FEAT_VIEWS, true, false, false, "wpt_pathtrace, views, all features, moving scenes, counting"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_VIEWS, false, false, false, "wpt_pathtrace, views, measured BRDFs"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_VIEWS, true, false, false, "wpt_pathtrace, views, measured BRDFs, counting"),
    /* adaptive sampling (args.adaptive): one pass, no counting builds */
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_ADAPTIVE, false, true, false, "wpt_pathtrace, adaptive, scene in LDS"),
    WPT_KERNEL_ROW(FEAT_BASIC | FEAT_ADAPTIVE, false, false, false, "wpt_pathtrace, adaptive, basic"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ADAPTIVE, false, false, false, "wpt_pathtrace, adaptive, all features"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_ANIM | FEAT_ADAPTIVE, false, false, false, "wpt_pathtrace, adaptive, all features, moving scenes"),
    WPT_KERNEL_ROW(FEAT_ALL | FEAT_RGL | FEAT_ANIM | FEAT_ADAPTIVE, false, false, false, "wpt_pathtrace, adaptive, measured BRDFs"),
};
#undef WPT_KERNEL_ROW
constexpr uint32_t KERNEL_TABLE_ROWS = sizeof(KERNEL_TABLE) / sizeof(KERNEL_TABLE[0]);

/* the row of an instantiation, or NULL: there is no such kernel */
inline const KernelEntry* findKernel(uint32_t features, bool count, bool ldsScene, bool wide)
{
    for (const KernelEntry& k : KERNEL_TABLE)
        if (k.features == features && k.count == count && k.ldsScene == ldsScene && k.wide == wide)
            return &k;
    return nullptr;
}

enum Sensor : uint32_t { SENSOR_FRAME, SENSOR_TRANSIENT, SENSOR_VIEWS, SENSOR_ADAPTIVE, SENSOR_TOF, SENSOR_COUNT };

struct KernelFacts {
    uint32_t need; /* feature bits of the scene and the launch's cameras, FEAT_ANIM folded in */
    Sensor sensor;
    bool count; /* the launch counts its work */
    uint32_t nodeCount, triCount, materialCount;
    bool sceneHasWide; /* the scene was uploaded with the collapsed tree as well (WPT_WALK_WIDE) */
    uint32_t variant;  /* wpt_set_launch_config */
    uint32_t walk;     /* wpt_set_walk */
};

struct KernelChoice {
    uint32_t features; /* the table key: findKernel(features, count, ldsScene, wide) */
    bool count, ldsScene, wide;
    bool basic;      /* the launch needs nothing beyond the basic feature set */
    bool sceneInLds; /* Cornell class at rest: the scene fits LDS and the sensor's kernel that keeps it there exists */
    bool rotated;    /* the scene's corners are in LDS in all three rotations (wpt_kernel_form: "rotated corners") */
    uint32_t materialsInLds; /* KernelArgs::materialsInLds */
    size_t sceneLdsBytes;    /* the launcher's: scene, rotated copies and material records as far as they are in LDS; 0 from HBM */
};

inline KernelChoice selectKernel(const KernelFacts& f)
{
    const bool frame = f.sensor == SENSOR_FRAME, tof = f.sensor == SENSOR_TOF, count = f.count;
    /* low bits of the variant word: 1 = keep the scene in HBM, 2 = all features */
    const uint32_t force = f.variant & 0x3u;
    const bool rgl = (f.need & FEAT_RGL) != 0; /* measured BRDFs have their own instantiations */
    const bool anim = (f.need & FEAT_ANIM) != 0;
    const size_t sceneBytes = size_t(f.nodeCount) * 32 + size_t(f.triCount) * 48;
    const size_t ldsBytes = sceneBytes + 32; /* the LDS copy: nodes, the null node, triangles */
    const bool lds = sceneBytes <= LDS_SCENE_MAX_BYTES && force != 1;
    /* (the time-of-flight kernel with the scene in LDS knows spot lights and two-sided materials besides) */
    const bool basic = (f.need & ~(tof ? FEAT_BASIC | FEAT_SPOT | FEAT_TWOSIDED : FEAT_BASIC)) == 0 && force != 2;
    const bool ldsSensor = basic && lds && !anim && !rgl;
    /* the wide walk where the scene has that form: product launches of the kernels that fetch the scene from HBM; counting
     * launches, moving scenes and the kernel with the scene in LDS walk the binary tree */
    const bool wide = f.sceneHasWide && frame && !count && !anim && !(basic && lds);
    /* The corners in LDS three times, once per rotation of (x, y, z), so that a triangle test reads them in its ray's component
     * order and selects nothing by axis (wpt_triangle.h, triangleTestRotated): plain product launches of the kernel with the scene in
     * LDS, where the two extra copies still leave four workgroups per compute unit.  The copies come before the material records:
     * those then stay in HBM unless they fit as well (the Cornell box: 40 768 of 40 960 bytes with the copies; DESIGN.md section 4
     * has both measured).  wpt_set_walk(WPT_WALK_SELECT_CORNERS) keeps the kernel that selects. */
    const size_t rotatedBytes = ldsBytes + 2 * size_t(f.triCount) * 48;
    const bool rotated = frame && ldsSensor && !count && !(f.walk & WPT_WALK_SELECT_CORNERS)
            && COLD_BYTES + rotatedBytes <= LDS_BYTES_PER_WORKGROUP_AT_FOUR;

    KernelChoice c = {};
    c.basic = basic;
    c.sceneInLds = ldsSensor;
    c.rotated = rotated;
    c.count = count;
    const uint32_t all = rgl ? FEAT_ALL | FEAT_RGL | FEAT_ANIM : anim ? FEAT_ALL | FEAT_ANIM : FEAT_ALL; /* the sensors' kernels from HBM */
    switch (f.sensor) {
    case SENSOR_TOF:
    case SENSOR_TRANSIENT: {
        const uint32_t sensor = tof ? FEAT_TOF : FEAT_TRANSIENT;
        c.ldsScene = ldsSensor;
        c.features = sensor | (ldsSensor ? (tof ? FEAT_BASIC | FEAT_TWOSIDED | FEAT_SPOT : FEAT_BASIC) : all);
        break;
    }
    case SENSOR_ADAPTIVE:
    case SENSOR_VIEWS: /* the kernel of the scene kind as for one frame; the views' kernel with the scene in LDS has no counting build */
        c.ldsScene = ldsSensor && !count;
        c.features = (f.sensor == SENSOR_VIEWS ? FEAT_VIEWS : FEAT_ADAPTIVE) | (c.ldsScene ? FEAT_BASIC : (rgl || anim) ? all : basic ? FEAT_BASIC : FEAT_ALL);
        break;
    default:
        if (anim) {
            c.features = rgl ? FEAT_ALL | FEAT_RGL | FEAT_ANIM : FEAT_ALL | FEAT_ANIM;
        } else if (count) {
            c.features = basic ? FEAT_BASIC : rgl ? FEAT_ALL | FEAT_RGL : FEAT_ALL;
        } else if (rgl) {
            c.features = FEAT_ALL | FEAT_RGL;
            c.wide = wide;
        } else if (basic && lds) {
            c.features = rotated ? FEAT_BASIC | FEAT_ROTATED : FEAT_BASIC;
            c.ldsScene = true;
        } else if (wide) { /* also for the basic feature set: the wide walk exists in the all-features instantiations */
            c.features = FEAT_ALL;
            c.wide = true;
        } else {
            c.features = basic ? FEAT_BASIC : FEAT_ALL;
        }
        break;
    }
    /* the material records join the scene in LDS, behind the rotated copies, where a quarter of a compute unit's 160 KiB holds a
     * workgroup with them (variant bit 0x80: never) */
    const size_t materialBytes = size_t(f.materialCount) * sizeof(wpt_material);
    const size_t sceneLdsBytes = rotated ? rotatedBytes : ldsBytes;
    if (!(f.variant & 0x80u) && COLD_BYTES + sceneLdsBytes + materialBytes <= LDS_BYTES_PER_WORKGROUP_AT_FOUR)
        c.materialsInLds = LDS_MATERIALS;
    c.sceneLdsBytes = !c.ldsScene ? 0 : sceneLdsBytes + (c.materialsInLds ? materialBytes : 0);
    /* the LDS copy of the tree folds first children that repeat their parent's box (wpt_fold.h); wpt_set_walk(WPT_WALK_NO_FOLD)
     * keeps every node's own first child */
    if (!(f.walk & WPT_WALK_NO_FOLD))
        c.materialsInLds |= LDS_FOLD;
    return c;
}

/* The large form (wpt_pathtrace_large): a decision of the launch on top of the choice above, which stays what it reports.  A
 * launch of the kernel with rotated corners runs as one workgroup of WG_LARGE lanes per compute unit, with the node array once
 * per sign octant behind the scene, where the scene has those copies (every box of its tree has lo <= hi: hasOrderedCopies), no
 * bound is NaN, the request fits what one workgroup may declare, and wpt_set_walk(WPT_WALK_SMALL_WORKGROUPS) does not keep the
 * workgroups of WG lanes.  Behind the node copies such a launch keeps what of a hit's data still fits in front of the cold words
 * (wpt_lds_places.h, hitDataPlaces and hitDataKernelParts; wpt_set_walk(WPT_WALK_HIT_DATA_IN_HBM): nothing of it); that never
 * decides the form.
 * counts: the scene's triangles, the instances its transformed triangles name (wpt_scene::normalsNamed) and its hot spots.
 * *sceneLdsBytes: the large launcher's; *hitData: what the launch adds to KernelArgs::materialsInLds, the parts in LDS and with
 * the normal matrices their number. */
struct HitDataCounts {
    uint32_t triCount, materialCount, instanceCount, hotspotCount;
};
inline bool selectLargeForm(const KernelChoice& c, uint32_t walk, bool hasOrderedCopies, bool boxesMayBeNan, uint32_t nodeCount, const HitDataCounts& counts,
        size_t* sceneLdsBytes, uint32_t* hitData)
{
    size_t bytes = c.sceneLdsBytes;
    if (LARGE_ORDERED) {
        uint32_t base, stride;
        const uint32_t nodeQuads = 2 * nodeCount + 2;
        bytes = size_t(orderedPlaces(nodeQuads, uint32_t(c.sceneLdsBytes / 16) - nodeQuads, base, stride)) * 16;
    }
    const bool large = c.rotated && c.ldsScene && c.features == (FEAT_BASIC | FEAT_ROTATED) && !(walk & WPT_WALK_SMALL_WORKGROUPS) && hasOrderedCopies
            && !boxesMayBeNan && COLD_BYTES_LARGE + bytes <= LDS_BYTES_PER_CU;
    *hitData = 0;
    if (large && !(walk & WPT_WALK_HIT_DATA_IN_HBM)) {
        const HitDataPlaces places = hitDataPlaces(nodeCount, counts.triCount, (c.materialsInLds & LDS_MATERIALS) ? counts.materialCount : 0u,
                counts.instanceCount, counts.hotspotCount, LARGE_ORDERED);
        /* (the function's own count of the scene in front of the parts is the launcher's: otherwise the parts stay out) */
        const uint32_t parts = hitDataKernelParts(places.parts); /* the kernels exist for three sets of parts */
        if (parts && size_t(places.nodeCopiesEnd) * 16 == bytes) {
            const uint32_t end = (parts & HIT_DATA_NORMALS) ? places.quads : places.normalsAt;
            /* ... and the material records by LDS address where they have a place: a bit of the launch's word beside the parts */
            const MaterialPlaces materials = materialPlaces(nodeCount, counts.triCount, counts.materialCount, (c.materialsInLds & LDS_MATERIALS) != 0, end);
            bytes = size_t(materials.quads) * 16;
            /* ... and with them the launch record, where what the scene keeps in LDS ends in front of its place: one more bit */
            const uint32_t record = materials.in && launchRecordFits(materials.quads) ? HIT_DATA_LAUNCH : 0u;
            *hitData = ((parts | (materials.in ? HIT_DATA_MATERIALS : 0u) | record) << LDS_HIT_DATA_SHIFT)
                    | ((parts & HIT_DATA_NORMALS) ? counts.instanceCount << LDS_HIT_NORMALS_SHIFT : 0u);
        }
    }
    *sceneLdsBytes = bytes;
    return large;
}

} /* namespace wptk */

#endif
