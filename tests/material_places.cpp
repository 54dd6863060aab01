/*
 * material_places.cpp -- wptk::materialPlaces and wptk::launchMaterialPlaces (wurblpt_amd/csrc/wpt_lds_places.h) as a program of
 * its own: where a launch in the large form of the rotated kernels keeps the material records that its kernel reads by LDS
 * address -- behind the corners where they are in LDS anyway, else behind the launch's parts of a hit's data, in front of the
 * paths' cold words.
 *
 *   material_places places NODES TRIANGLES MATERIALS BEHIND_CORNERS INSTANCES HOTSPOTS
 *       one line: in at quads kernelParts end   (tests/test_material_places.py holds rows to it; end: where the kernel's parts of a
 *       hit's data end, hitDataPlaces' own; kernelParts: hitDataKernelParts)
 *   material_places sweep CASES
 *       CASES random counts, and every count of the small ones: each result is checked against the rules written out below, which
 *       restate nothing of the function's arithmetic but what a layout must satisfy; hitDataPlaces and hitDataKernelParts are
 *       held to the rows they returned before there were material records behind them.
 *
 * g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Werror tests/material_places.cpp -o material_places
 */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../wurblpt_amd/csrc/wpt_lds_places.h"

using namespace wptk;

namespace {

constexpr uint64_t ROOM = (32 * 1024 - 512) / 16; /* quadwords between the math tables and the cold words at 32 KiB */
constexpr uint64_t MATERIAL_QUADS = sizeof(wpt_material) / 16;

uint64_t g_violations = 0;
uint64_t g_inBehindParts = 0, g_inBehindCorners = 0, g_noRoom = 0, g_noKernel = 0, g_noMaterials = 0, g_tooLarge = 0, g_lastQuad = 0, g_firstBehind = 0;

void violation(const char* what, uint32_t n, uint32_t t, uint32_t m, bool b, uint32_t i, uint32_t h)
{
    if (g_violations++ < 20)
        fprintf(stderr, "violation: %s (nodes %u triangles %u materials %u behind corners %d instances %u hot spots %u)\n", what, n, t, m, int(b), i, h);
}

struct Range {
    uint64_t from, to; /* [from, to) in quadwords from the scene's start */
};

bool disjoint(Range a, Range b)
{
    return a.to <= b.from || b.to <= a.from || a.from == a.to || b.from == b.to;
}

/* where the parts of a hit's data that the launch's kernel has end; false: there is no such kernel, or the scene is beyond the room */
bool kernelEnd(uint32_t n, uint32_t t, uint32_t inFront, uint32_t i, uint32_t h, uint32_t& parts, uint64_t& end, HitDataPlaces& p)
{
    p = hitDataPlaces(n, t, inFront, i, h);
    parts = hitDataKernelParts(p.parts);
    end = (parts & HIT_DATA_NORMALS) ? p.quads : p.normalsAt;
    return parts != 0;
}

void check(uint32_t n, uint32_t t, uint32_t m, bool b, uint32_t i, uint32_t h)
{
    auto bad = [&](const char* what) { violation(what, n, t, m, b, i, h); };
    uint32_t parts = 0xffffffffu;
    const MaterialPlaces mp = launchMaterialPlaces(n, t, m, b, i, h, &parts);
    const MaterialPlaces again = launchMaterialPlaces(n, t, m, b, i, h);
    if (again.in != mp.in || again.at != mp.at || again.quads != mp.quads)
        bad("two calls differ");
    uint32_t kernel;
    uint64_t end;
    HitDataPlaces p;
    const bool haveKernel = kernelEnd(n, t, b ? m : 0u, i, h, kernel, end, p);
    if (parts != kernel)
        bad("the kernel's parts are not hitDataKernelParts'");
    const uint64_t nodeQuads = 2ull * n + 2, corners = 9ull * t, need = MATERIAL_QUADS * m;
    if (nodeQuads + corners + (b ? need : 0) > ROOM)
        g_tooLarge++;
    if (!haveKernel) { /* a kernel without parts reads the records like every other kernel */
        g_noKernel++;
        if (mp.in)
            bad("material records by LDS address for a kernel without parts");
        return;
    }
    if (end > ROOM)
        bad("the kernel's parts end behind the room");
    if (m == 0) {
        g_noMaterials++;
        if (mp.in || mp.quads != end)
            bad("a scene without materials has records in, or grows");
        return;
    }
    /* what lies in front: copy 0 of the nodes, the corners (with the materials, where they follow them), copies 1 .. 7, the parts */
    uint32_t base, stride;
    orderedPlaces(uint32_t(nodeQuads), uint32_t(corners + (b ? need : 0)), base, stride);
    const Range nodes = { 0, nodeQuads }, cornerRange = { nodeQuads, nodeQuads + corners }, partsRange = { p.nodeCopiesEnd, end };
    if (b) {
        /* already in LDS behind the corners: read there, nothing added */
        if (!mp.in || mp.at != nodeQuads + corners || mp.quads != end)
            bad("records behind the corners are not read where they lie");
        g_inBehindCorners++;
    } else {
        const bool fits = end + need <= ROOM;
        if (mp.in != fits)
            bad(fits ? "records that fit behind the parts are not in" : "records are in that end behind the room");
        if (mp.at != end)
            bad("the records do not start where the parts end");
        if (mp.quads != (fits ? end + need : end))
            bad("the whole does not end behind what is in");
        g_inBehindParts += fits;
        g_noRoom += !fits;
        g_lastQuad += fits && end + need == ROOM;
        g_firstBehind += !fits && end + need <= ROOM + MATERIAL_QUADS;
    }
    if (mp.in) {
        const Range r = { mp.at, mp.at + need };
        if (r.to > ROOM || mp.quads > ROOM)
            bad("the records overlap the cold words");
        if (!disjoint(r, nodes) || !disjoint(r, cornerRange) || (!b && !disjoint(r, partsRange)))
            bad("the records overlap the nodes, the corners or the parts");
        for (uint32_t k = 1; k < ORDERED_COPIES; k++) {
            const Range copy = { uint64_t(base) + uint64_t(k) * stride, uint64_t(base) + uint64_t(k) * stride + nodeQuads };
            if (!disjoint(r, copy))
                bad("the records overlap a node copy");
        }
    }
}

/* hitDataPlaces and hitDataKernelParts as they were: rows of tests/test_hit_data_layout.py, written out again */
void checkExisting()
{
    struct Row {
        uint32_t n, t, m, i, h;
        HitDataPlaces p;
        uint32_t kernel;
    };
    static const Row rows[] = {
        { 71, 36, 0, 0, 2, { 3, 1504, 1756, 1772, 1504, 1772 }, 3 },
        { 71, 36, 0, 18, 2, { 7, 1504, 1756, 1772, 1504, 1826 }, 7 },
        { 71, 36, 6, 18, 2, { 7, 1552, 1804, 1820, 1552, 1874 }, 7 },
        { 71, 36, 0, 82, 2, { 3, 1504, 1756, 1772, 1504, 1772 }, 3 },
        { 71, 36, 0, 4, 31, { 7, 1504, 1756, 2004, 1504, 2016 }, 7 },
        { 71, 36, 0, 1, 33, { 1, 1504, 1756, 1756, 1504, 1756 }, 0 },
        { 101, 36, 0, 18, 2, { 0, 2000, 2000, 2000, 2000, 2000 }, 0 },
        { 3, 1, 0, 65536, 1, { 3, 144, 151, 159, 144, 159 }, 3 },
    };
    for (const Row& r : rows) {
        const HitDataPlaces p = hitDataPlaces(r.n, r.t, r.m, r.i, r.h);
        if (p.parts != r.p.parts || p.recordsAt != r.p.recordsAt || p.hotspotsAt != r.p.hotspotsAt || p.normalsAt != r.p.normalsAt
                || p.nodeCopiesEnd != r.p.nodeCopiesEnd || p.quads != r.p.quads || hitDataKernelParts(p.parts) != r.kernel)
            violation("hitDataPlaces or hitDataKernelParts returns something else than before", r.n, r.t, r.m, false, r.i, r.h);
    }
    if (HIT_DATA_RECORDS != 1 || HIT_DATA_HOTSPOTS != 2 || HIT_DATA_NORMALS != 4 || HIT_DATA_ALL != 7 || HIT_RECORD_QUADS != 7 || HIT_HOTSPOT_QUADS != 8
            || HIT_NORMAL_QUADS != 3 || (HIT_DATA_MATERIALS & HIT_DATA_ALL) != 0)
        violation("the parts' values have changed", 0, 0, 0, false, 0, 0);
}

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t below)
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return uint32_t((g_state >> 20) % below);
}

} /* namespace */

int main(int argc, char** argv)
{
    if (argc == 8 && !strcmp(argv[1], "places")) {
        uint32_t v[6];
        for (int k = 0; k < 6; k++)
            v[k] = uint32_t(strtoul(argv[2 + k], nullptr, 10));
        uint32_t parts = 0, kernel;
        uint64_t end;
        HitDataPlaces p;
        const MaterialPlaces mp = launchMaterialPlaces(v[0], v[1], v[2], v[3] != 0, v[4], v[5], &parts);
        kernelEnd(v[0], v[1], v[3] ? v[2] : 0u, v[4], v[5], kernel, end, p);
        printf("%d %u %u %u %" PRIu64 "\n", int(mp.in), mp.at, mp.quads, parts, end);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "sweep")) {
        const uint64_t cases = strtoull(argv[2], nullptr, 10);
        uint64_t done = 0;
        checkExisting();
        /* every count of the small ones, then random counts of the sizes that fit LDS, then counts of any size */
        for (uint32_t n = 1; n <= 9; n += 4)
            for (uint32_t t = 0; t <= 3; t++)
                for (uint32_t m = 0; m <= 2; m++)
                    for (uint32_t b = 0; b <= 1; b++)
                        for (uint32_t i = 0; i <= 1; i++)
                            for (uint32_t h = 0; h <= 2; h++, done++)
                                check(n, t, m, b != 0, i, h);
        for (; done < cases; done++) {
            const uint32_t kind = draw(8);
            if (kind == 0) {
                const uint32_t huge[4] = { 0xffffffffu, 0x80000000u, 0x10000u, 70000u };
                check(draw(2) ? huge[draw(4)] : draw(400), draw(2) ? huge[draw(4)] : draw(200), draw(2) ? huge[draw(4)] : draw(40), draw(2) != 0,
                        draw(2) ? huge[draw(4)] : draw(300), draw(2) ? huge[draw(4)] : draw(60));
            } else if (kind <= 2) { /* near the room's end: the Cornell box's size with the records sized to the quadword */
                const uint32_t h = 1 + draw(12), i = draw(2) ? draw(20) : 0;
                uint32_t parts;
                uint64_t end;
                HitDataPlaces p;
                if (!kernelEnd(71, 36, 0, i, h, parts, end, p))
                    continue;
                const uint32_t left = uint32_t(ROOM - end) / uint32_t(MATERIAL_QUADS);
                check(71, 36, left + draw(3) - (left ? 1 : 0), false, i, h);
            } else {
                check(1 + draw(160), draw(90), draw(4) ? draw(40) : 0, draw(3) == 0, draw(3) ? draw(120) : 0, draw(4) ? draw(24) : 0);
            }
        }
        printf("cases %" PRIu64 ", violations %" PRIu64 "\n", done, g_violations);
        printf("records in behind the parts: %" PRIu64 " (ending with the room's last quadword: %" PRIu64 "), behind the corners: %" PRIu64
               ", no room: %" PRIu64 " (by one record or less: %" PRIu64 ")\n", g_inBehindParts, g_lastQuad, g_inBehindCorners, g_noRoom, g_firstBehind);
        printf("kernels without parts: %" PRIu64 ", scenes without materials: %" PRIu64 ", scenes beyond the room: %" PRIu64 "\n", g_noKernel, g_noMaterials, g_tooLarge);
        const bool covered = g_inBehindParts > 0 && g_lastQuad > 0 && g_inBehindCorners > 0 && g_noRoom > 0 && g_firstBehind > 0 && g_noKernel > 0
                && g_noMaterials > 0 && g_tooLarge > 0;
        printf("cases covered: %s\n", covered ? "yes" : "NO");
        return g_violations == 0 && covered ? 0 : 1;
    }
    fprintf(stderr, "usage: %s places NODES TRIANGLES MATERIALS BEHIND_CORNERS INSTANCES HOTSPOTS | sweep CASES\n", argv[0]);
    return 2;
}
