/*
 * hit_data_layout.cpp -- wptk::hitDataPlaces (wurblpt_amd/csrc/wpt_lds_places.h) as a program of its own: where the large form of
 * the rotated kernels keeps a hit's data in LDS, behind the node copies and in front of the paths' cold words.
 *
 *   hit_data_layout places NODES TRIANGLES MATERIALS INSTANCES HOTSPOTS
 *       one line: parts recordsAt hotspotsAt normalsAt nodeCopiesEnd quads kernelParts   (tests/test_hit_data_layout.py holds rows
 *       to it; kernelParts: hitDataKernelParts, the parts of the kernel a launch runs)
 *   hit_data_layout sweep CASES
 *       CASES random counts, and every count of the small ones: each result is checked against the rules written out below, which
 *       restate nothing of the function's arithmetic but what a layout must satisfy.
 *
 * g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Werror tests/hit_data_layout.cpp -o hit_data_layout
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
uint64_t g_seen[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
uint64_t g_stopped = 0, g_empty = 0, g_tooLarge = 0;

void violation(const char* what, uint32_t n, uint32_t t, uint32_t m, uint32_t i, uint32_t h)
{
    if (g_violations++ < 20)
        fprintf(stderr, "violation: %s (nodes %u triangles %u materials %u instances %u hot spots %u)\n", what, n, t, m, i, h);
}

struct Range {
    uint64_t from, to; /* [from, to) in quadwords from the scene's start */
};

bool disjoint(Range a, Range b)
{
    return a.to <= b.from || b.to <= a.from || a.from == a.to || b.from == b.to;
}

void check(uint32_t n, uint32_t t, uint32_t m, uint32_t i, uint32_t h)
{
    const HitDataPlaces p = hitDataPlaces(n, t, m, i, h);
    const uint64_t nodeQuads = 2ull * n + 2, behind = 9ull * t + MATERIAL_QUADS * m;
    auto bad = [&](const char* what) { violation(what, n, t, m, i, h); };
    if (hitDataPlaces(n, t, m, i, h).parts != p.parts || hitDataPlaces(n, t, m, i, h).quads != p.quads)
        bad("two calls differ");
    if (nodeQuads + behind > ROOM) { /* the scene alone is beyond the room: nothing is promised but that nothing is in */
        g_tooLarge++;
        if (p.parts != 0)
            bad("parts for a scene that does not fit");
        return;
    }
    /* the scene in front: copy 0 with corners and materials, copies 1 .. 7 where orderedPlaces says */
    uint32_t base, stride;
    const uint32_t end = orderedPlaces(uint32_t(nodeQuads), uint32_t(behind), base, stride);
    if (p.nodeCopiesEnd != end)
        bad("nodeCopiesEnd is not orderedPlaces'");
    const Range front = { 0, nodeQuads + behind };
    Range copies[ORDERED_COPIES];
    for (uint32_t k = 1; k < ORDERED_COPIES; k++) {
        copies[k] = { uint64_t(base) + uint64_t(k) * stride, uint64_t(base) + uint64_t(k) * stride + nodeQuads };
        if (!disjoint(copies[k], front) || copies[k].to > end)
            bad("a node copy overlaps the corners or the materials, or ends behind the whole");
        if (k > 1 && !disjoint(copies[k], copies[k - 1]))
            bad("two node copies overlap");
    }
    /* the parts: in the order records, hot spots, normal matrices, each behind everything before it and in front of the cold words */
    const uint64_t size[3] = { 7ull * t, 8ull * h, 3ull * i };
    const uint32_t bit[3] = { HIT_DATA_RECORDS, HIT_DATA_HOTSPOTS, HIT_DATA_NORMALS };
    const uint32_t at[3] = { p.recordsAt, p.hotspotsAt, p.normalsAt };
    uint64_t next = end;
    bool open = end <= ROOM, stopped = false;
    for (int k = 0; k < 3; k++) {
        if (at[k] != next)
            bad("a part does not start where the one before ends");
        const bool in = (p.parts & bit[k]) != 0;
        if (size[k] == 0) {
            if (in)
                bad("a part with nothing to hold is in");
            continue;
        }
        const bool fits = open && next + size[k] <= ROOM && (k != 2 || i <= 0xffffu);
        if (in != fits)
            bad(fits ? "a part that fits behind the parts before it is not in" : "a part is in that does not fit, or that follows one that did not");
        if (in) {
            const Range r = { next, next + size[k] };
            if (r.from < end || r.to > ROOM || !disjoint(r, front))
                bad("a part overlaps the scene or the cold words");
            for (uint32_t c = 1; c < ORDERED_COPIES; c++)
                if (!disjoint(r, copies[c]))
                    bad("a part overlaps a node copy");
            next = r.to;
        } else {
            open = false;
            stopped = true;
        }
    }
    if (p.quads != next)
        bad("the whole does not end where the last part ends");
    if (p.parts && p.quads > ROOM)
        bad("the whole overlaps the cold words");
    /* the kernel a launch runs has parts that all fit: all three, records and hot spots, or none */
    const uint32_t kernel = hitDataKernelParts(p.parts);
    if ((kernel & ~p.parts) || (kernel != 0 && kernel != 3 && kernel != 7) || (p.parts == 7 && kernel != 7) || ((p.parts & 3) == 3 && kernel == 0))
        bad("the kernel's parts are not the largest of the three sets that fits");
    g_seen[p.parts & 7]++;
    g_stopped += stopped;
    g_empty += (t == 0 || h == 0 || i == 0);
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
    if (argc == 7 && !strcmp(argv[1], "places")) {
        uint32_t v[5];
        for (int k = 0; k < 5; k++)
            v[k] = uint32_t(strtoul(argv[2 + k], nullptr, 10));
        const HitDataPlaces p = hitDataPlaces(v[0], v[1], v[2], v[3], v[4]);
        printf("%u %u %u %u %u %u %u\n", p.parts, p.recordsAt, p.hotspotsAt, p.normalsAt, p.nodeCopiesEnd, p.quads, hitDataKernelParts(p.parts));
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "sweep")) {
        const uint64_t cases = strtoull(argv[2], nullptr, 10);
        uint64_t done = 0;
        /* every count of the small ones, then random counts of the sizes that fit LDS, then counts of any size */
        for (uint32_t n = 1; n <= 9; n += 4)
            for (uint32_t t = 0; t <= 3; t++)
                for (uint32_t m = 0; m <= 2; m++)
                    for (uint32_t i = 0; i <= 2; i++)
                        for (uint32_t h = 0; h <= 2; h++, done++)
                            check(n, t, m, i, h);
        for (; done < cases; done++) {
            const uint32_t kind = draw(8);
            if (kind == 0) {
                const uint32_t huge[4] = { 0xffffffffu, 0x80000000u, 0x10000u, 70000u };
                check(draw(2) ? huge[draw(4)] : draw(400), draw(2) ? huge[draw(4)] : draw(200), draw(2) ? huge[draw(4)] : draw(40),
                        draw(2) ? huge[draw(4)] : draw(300), draw(2) ? huge[draw(4)] : draw(60));
            } else if (kind == 1) { /* near the room's end: the Cornell box's size with the last part sized to the quadword */
                const uint32_t h = draw(12);
                const HitDataPlaces p = hitDataPlaces(71, 36, 0, 0, h);
                const uint32_t left = uint32_t(ROOM) - p.quads;
                check(71, 36, 0, left / 3 + draw(3) - (left / 3 ? 1 : 0), h);
            } else {
                check(1 + draw(160), draw(90), draw(3) ? draw(12) : 0, draw(3) ? draw(120) : 0, draw(4) ? draw(24) : 0);
            }
        }
        printf("cases %" PRIu64 ", violations %" PRIu64 "\n", done, g_violations);
        printf("parts seen: none %" PRIu64 ", 1: %" PRIu64 ", 2: %" PRIu64 ", 3: %" PRIu64 ", 4: %" PRIu64 ", 5: %" PRIu64 ", 6: %" PRIu64 ", 7: %" PRIu64 "\n",
                g_seen[0], g_seen[1], g_seen[2], g_seen[3], g_seen[4], g_seen[5], g_seen[6], g_seen[7]);
        printf("a part did not fit: %" PRIu64 ", a part had nothing to hold: %" PRIu64 ", scenes beyond the room: %" PRIu64 "\n", g_stopped, g_empty, g_tooLarge);
        bool covered = g_stopped > 0 && g_empty > 0 && g_tooLarge > 0;
        for (int k = 0; k < 8; k++)
            covered = covered && g_seen[k] > 0;
        printf("cases covered: %s\n", covered ? "yes" : "NO");
        return g_violations == 0 && covered ? 0 : 1;
    }
    fprintf(stderr, "usage: %s places NODES TRIANGLES MATERIALS INSTANCES HOTSPOTS | sweep CASES\n", argv[0]);
    return 2;
}
