/*
 * wpt_lds_places.h -- where the large form of the rotated kernels keeps what in a compute unit's LDS (host and device; no HIP
 * header, nothing global: wpt_scene_layout.h includes it for the host, wpt_pathtrace.inc.h for the kernels and the launch, and
 * tests/hit_data_layout.cpp and tests/material_places.cpp compile it on their own under the host sanitizers).
 *
 *   [ math tables ][ nodes, null node | corners x 3 | materials ][ node copies 1 .. 7 ][ hit data ][ materials ] ... [ cold words at 32 KiB ]
 *
 * orderedPlaces says where the node copies lie, hitDataPlaces what of a hit's data follows them and where, materialPlaces where
 * the material records are read by LDS address (in either of the two places, never both).  All places are
 * quadwords (16 bytes) from the scene's start, which lies behind the math tables.
 */
#ifndef WPT_LDS_PLACES_H
#define WPT_LDS_PLACES_H

#include <stdint.h>

#include "../../include/wurblpt_hip.h"

#if defined(__HIPCC__)
#define WPT_PLACES_FN __host__ __device__ inline
#else
#define WPT_PLACES_FN inline
#endif

namespace wptk {

constexpr uint32_t ORDERED_COPIES = 8; /* node arrays of the ordered form, one per sign octant */
/* Where the ordered form's node arrays lie in LDS, in quadwords from copy 0 (host and device).  nodeQuads: a copy with its null
 * node; behind: corners and material records, which follow copy 0.  Copy k >= 1 lies at base + k * stride, behind all that, with
 * base a multiple of 16 quadwords and stride 2 more than one: the eight records of a node then lie 32 bytes apart modulo the 256
 * bytes of the LDS's 64 banks.  Lanes of a wave that stand on one node in different octants so read different banks; with the
 * copies back to back a copy of the Cornell box's tree is 2304 bytes, nine times 256, and they read the same ones (measured:
 * five times the parent's bank conflict cycles).  Returns the quadwords of the whole. */
WPT_PLACES_FN uint32_t orderedPlaces(uint32_t nodeQuads, uint32_t behind, uint32_t& base, uint32_t& stride)
{
    const uint32_t used = nodeQuads + behind;
    stride = ((nodeQuads + 13u) & ~15u) + 2u;
    base = used > stride ? ((used - stride + 15u) & ~15u) : 0u;
    return base + ORDERED_COPIES * stride;
}

/* ---- a hit's data in LDS (wpt_pathtrace_body.inc.h copies it there, LdsHitData of wpt_device.h reads it) ----
 * What the long round of a path would otherwise fetch from global memory, in three parts:
 *   HIT_DATA_RECORDS   per triangle HIT_RECORD_QUADS quadwords: the six attribute quadwords of SceneView::triAttr, then
 *                      (instance, material, flags, 0) from the triangle's record in SceneView::triGeom.  Seven and not eight:
 *                      lanes gather different triangles at once, and with an odd stride sixteen neighbouring triangles start in
 *                      sixteen different groups of four banks, with eight in two.
 *   HIT_DATA_HOTSPOTS  per hot spot HIT_HOTSPOT_QUADS quadwords: its face (SceneView::hotspotFace) | prim transform p0.x p0.y |
 *                      p0.z p1.x p1.y p1.z | p2.x p2.y p2.z 0 | the four columns of M.  The pdf loop reads the first and the
 *                      first word of the second at a wave-uniform place; the light sample reads the rest, each lane its own.
 *   HIT_DATA_NORMALS   per instance HIT_NORMAL_QUADS quadwords: the three columns of wpt_instance::N, a spare word behind
 *                      each, for instances 0 .. instanceCount - 1.
 * The parts follow the node copies in the order records, hot spots, normal matrices, as long as they end in front of the cold
 * words.  A part that has nothing to hold is not in, and the next one is asked; a part that does not fit is not in, and neither
 * is what follows it: the order is that of what a part saves.  What is not in stays in HBM. */
constexpr uint32_t HIT_DATA_RECORDS = 1u, HIT_DATA_HOTSPOTS = 2u, HIT_DATA_NORMALS = 4u;
constexpr uint32_t HIT_RECORD_QUADS = 7, HIT_HOTSPOT_QUADS = 8, HIT_NORMAL_QUADS = 3;
/* the scene's room in the large form: from behind the math tables (512 bytes) to the cold words at 32 KiB
 * (wpt_pathtrace.inc.h asserts that these are TABLE_BYTES and COLD_AT_LARGE) */
constexpr uint32_t LARGE_SCENE_ROOM_QUADS = (32u * 1024u - 512u) / 16u;
/* the most instances HIT_DATA_NORMALS takes: their number travels in the upper half of KernelArgs::materialsInLds */
constexpr uint32_t HIT_NORMALS_MAX = 0xffffu;
constexpr uint32_t HIT_DATA_ALL = HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS | HIT_DATA_NORMALS;
/* The parts are template arguments of the kernels (LdsHitData), and the library has the large form for three sets of them: all
 * three, records and hot spots (a scene without transformed triangles: the Cornell box), and none.  A launch runs the largest
 * of these whose parts all fit; `fit`: hitDataPlaces' parts. */
WPT_PLACES_FN uint32_t hitDataKernelParts(uint32_t fit)
{
    const uint32_t two = HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS;
    return (fit & HIT_DATA_ALL) == HIT_DATA_ALL ? HIT_DATA_ALL : (fit & two) == two ? two : 0u;
}

struct HitDataPlaces {
    uint32_t parts;                            /* HIT_DATA_* of the parts that are in LDS */
    uint32_t recordsAt, hotspotsAt, normalsAt; /* where each part starts (where it is not in: where it would) */
    uint32_t nodeCopiesEnd;                    /* the quadwords of the scene without any part: orderedPlaces' */
    uint32_t quads;                            /* ... and with the parts that are in */
};

/* nodeCount, triCount: the tree and its triangles; materialCount: the material records IN LDS (0 where they stay in HBM);
 * instanceCount: the instances whose normal matrix a triangle with WPT_TRI_TRANSFORM names (0: there is none); hotspotCount:
 * the scene's hot spots, all triangles.  ordered: the launch walks ordered node copies (always, but for a measurement build).
 * Counts so large that the scene itself is far beyond the room give no parts; nothing here overflows for any input. */
WPT_PLACES_FN HitDataPlaces hitDataPlaces(uint32_t nodeCount, uint32_t triCount, uint32_t materialCount, uint32_t instanceCount, uint32_t hotspotCount,
        bool ordered = true)
{
    HitDataPlaces p = { 0u, 0u, 0u, 0u, 0u, 0u };
    const uint64_t nodeQuads64 = 2ull * nodeCount + 2ull;
    const uint64_t behind64 = 9ull * triCount + uint64_t(materialCount) * (sizeof(wpt_material) / 16);
    if (nodeQuads64 + behind64 > LARGE_SCENE_ROOM_QUADS) { /* (no launch in the large form has such a scene) */
        p.nodeCopiesEnd = p.quads = p.recordsAt = p.hotspotsAt = p.normalsAt = 0xffffffffu;
        return p;
    }
    const uint32_t nodeQuads = uint32_t(nodeQuads64), behind = uint32_t(behind64);
    uint32_t base, stride;
    p.nodeCopiesEnd = ordered ? orderedPlaces(nodeQuads, behind, base, stride) : nodeQuads + behind;
    uint32_t at = p.nodeCopiesEnd;
    bool open = at <= LARGE_SCENE_ROOM_QUADS;
    /* one part: `count` records of `each` quadwords (the counts are below 2^32 and `each` is small: 64 bits hold the product) */
    auto part = [&](uint32_t bit, uint64_t count, uint32_t each, uint32_t& where) {
        where = at;
        if (count == 0)
            return;
        if (open && at + count * each <= LARGE_SCENE_ROOM_QUADS) {
            p.parts |= bit;
            at += uint32_t(count * each);
        } else {
            open = false;
        }
    };
    part(HIT_DATA_RECORDS, triCount, HIT_RECORD_QUADS, p.recordsAt);
    part(HIT_DATA_HOTSPOTS, hotspotCount, HIT_HOTSPOT_QUADS, p.hotspotsAt);
    part(HIT_DATA_NORMALS, instanceCount <= HIT_NORMALS_MAX ? instanceCount : 0xffffffffull, HIT_NORMAL_QUADS, p.normalsAt);
    p.quads = at;
    return p;
}

/* ---- the material records by LDS address (the large form; LdsHitData::material reads them) ----
 * A launch whose kernel reads hit records and hot spots from LDS (hitDataKernelParts: not 0) reads the material records there
 * as well where they have a place, and then "the materials are in LDS" is a fact of the instantiation, HIT_DATA_MATERIALS among
 * its template argument's bits: the long round fetches a hit's material with LDS instructions at an offset from the scene's
 * start, not through a generic pointer that may as well point to HBM.  The bit is the kernels' and the launch word's own:
 * HIT_DATA_ALL, hitDataPlaces and what wpt_kernel_hit_data reports do not know it.
 * The records, whole (HIT_MATERIAL_QUADS quadwords each, as in HBM), have a place
 *   behind the corners, where the launch keeps them already (behindCorners: LDS_MATERIALS, and hitDataPlaces counted them), or
 *   at `end`, the quadword where the launch's scene and its parts of a hit's data end, if they end in front of the cold words.
 * Otherwise, and for a scene without materials, they are not in: the launch runs the kernel without the bit, which fetches them
 * through SceneView::materials like every other kernel. */
constexpr uint32_t HIT_DATA_MATERIALS = 8u;
constexpr uint32_t HIT_MATERIAL_QUADS = uint32_t(sizeof(wpt_material) / 16);

struct MaterialPlaces {
    bool in;        /* the kernel reads the material records by LDS address */
    uint32_t at;    /* where they start, in quadwords from the scene's start (not in: where they would) */
    uint32_t quads; /* the quadwords of the scene with them: `end`, or behind the records placed there */
};

/* nodeCount, triCount: as for hitDataPlaces; materialCount: the scene's material records; end: HitDataPlaces::quads of the parts
 * the launch's kernel has.  Nothing here overflows for any input. */
WPT_PLACES_FN MaterialPlaces materialPlaces(uint32_t nodeCount, uint32_t triCount, uint32_t materialCount, bool behindCorners, uint32_t end)
{
    MaterialPlaces p = { false, end, end };
    const uint64_t need = uint64_t(materialCount) * HIT_MATERIAL_QUADS;
    if (materialCount == 0 || end > LARGE_SCENE_ROOM_QUADS)
        return p;
    if (behindCorners) {
        const uint64_t at = 2ull * nodeCount + 2ull + 9ull * triCount;
        p.at = at <= LARGE_SCENE_ROOM_QUADS ? uint32_t(at) : 0xffffffffu;
        p.in = at + need <= end; /* (the node copies lie behind them: a launch in the large form has it so) */
        return p;
    }
    if (end + need <= LARGE_SCENE_ROOM_QUADS) {
        p.in = true;
        p.quads = uint32_t(end + need);
    }
    return p;
}

/* ---- the launch record (the large form; blockNewFrom reads it, wpt_blocks.h: LaunchRecordInLds) ----
 * What the new-sample block reads of a launch's constants, LAUNCH_RECORD_QUADS quadwords that the kernel's prologue writes: the
 * rays' origin and invSamplesSqrt | the frustum l r b t | the rotation | invWidth, invHeight, samplesSqrt, randomize_ray_over_pixel.
 * Its place does not depend on the scene: the last quadwords of the scene's room, straight in front of the cold words, so that no
 * part of the layout above moves for it and its address is a literal of the instruction.  A launch whose kernel reads the
 * material records by LDS address has it where those (materialPlaces' quads: the end of all the scene keeps in LDS) end in
 * front of it, and then the record is a fact of the instantiation like the records themselves, HIT_DATA_LAUNCH among its template
 * argument's bits; every other launch runs the kernel without the bit, whose block reads the arguments. */
constexpr uint32_t HIT_DATA_LAUNCH = 16u;
constexpr uint32_t LAUNCH_RECORD_QUADS = 4;
constexpr uint32_t LAUNCH_RECORD_AT = LARGE_SCENE_ROOM_QUADS - LAUNCH_RECORD_QUADS;
/* end: the quadwords of the launch's scene with all that follows it (MaterialPlaces::quads) */
WPT_PLACES_FN bool launchRecordFits(uint32_t end)
{
    return end <= LAUNCH_RECORD_AT;
}

/* The steps of a launch in the large form in one (selectLargeForm's, wpt_kernel_table.h): the parts that fit, the kernel's set of
 * them (*kernelParts, or NULL), and the material records behind what that kernel keeps.  A kernel without parts reads the
 * material records like every other kernel: they are not in. */
WPT_PLACES_FN MaterialPlaces launchMaterialPlaces(uint32_t nodeCount, uint32_t triCount, uint32_t materialCount, bool behindCorners, uint32_t instanceCount,
        uint32_t hotspotCount, uint32_t* kernelParts = nullptr)
{
    const HitDataPlaces places = hitDataPlaces(nodeCount, triCount, behindCorners ? materialCount : 0u, instanceCount, hotspotCount);
    const uint32_t parts = hitDataKernelParts(places.parts);
    if (kernelParts)
        *kernelParts = parts;
    if (!parts) {
        const MaterialPlaces none = { false, places.nodeCopiesEnd, places.nodeCopiesEnd };
        return none;
    }
    return materialPlaces(nodeCount, triCount, materialCount, behindCorners, (parts & HIT_DATA_NORMALS) ? places.quads : places.normalsAt);
}

} /* namespace wptk */

#endif
