/*
 * wpt_bypass.h -- inner nodes that the walk of a tree in LDS leaves out, and the link words that go round them (host only).
 *
 * A node's box test is a filter: what fixes a frame's bits is the sequence of triangle tests and the bound each runs under.
 * Take an inner node P whose two children's boxes lie within its own.  (bound - origin) * reciprocal is two correctly rounded
 * operations, each monotone in `bound`, so on every axis a child's slab interval lies within P's: a ray that fails P's test
 * under a bound B fails both children's under B -- provided the six slab distances are numbers, which is every ray for which
 * rayMayNan (wpt_device.h) is false and every box whose bounds are numbers.  The walk may therefore leave P out and go to its
 * first child wherever a link led to P: when P would have passed nothing changes; when P would have failed, the boxes tested
 * in its place are those of its nearest kept descendants, back to back with no leaf test between them, so the bound is B for
 * all of them, they all fail, and the walk arrives at P's skip link as before.  By induction any set R of such nodes may be
 * left out together.  The leaves tested, their order and every bound are the reference's; the node step is the same
 * instructions; the price is the extra failing tests on the rays that would have failed P.
 *
 * Rays that carry RAY_MAY_NAN are outside the argument (the reference's comparison chains depend on operand order there): the
 * kernels walk them over the exact links (the fold's, wpt_fold.h), which is sound from step to step because a lane that
 * stands on a node index has the same work ahead of it under both sets of links.  A tree with a NaN bound keeps the exact
 * links for every ray.
 *
 * Which eligible nodes go is a cost model's choice: a fixed, seeded sample of rays made from the scene itself (origins on its
 * triangles, directions into both half-spaces of the face; the description carries no camera) walks the tree as the reference does and counts, per node, the
 * tests that passed and failed.  The visits of a walk that leaves R out follow from those counts in closed form (visits()
 * below), and a local search adds nodes to R while the visits fall.  The plan never has more visits on its sample than the
 * folded walk, and it is a pure function of the tree and the triangles.
 */
#ifndef WPT_BYPASS_H
#define WPT_BYPASS_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/wurblpt_hip.h"
#include "wpt_fold.h"

namespace wptb {

constexpr uint32_t NODE_CHILD = wptf::FOLD_NODE_CHILD, NODE_INDEX_MASK = wptf::FOLD_INDEX_MASK;
constexpr uint32_t PRIM_SPHERE_BIT = 0x80000000u;
constexpr uint32_t SAMPLE_RAYS = 4096;     /* rays of the cost model's sample */
constexpr uint32_t SEARCH_PASSES_MAX = 8;  /* passes of the local search over the eligible nodes */
constexpr uint32_t MODE_MODEL = 0, MODE_ALL_ELIGIBLE = 1;

/* device nodes, eight words each (wpt_scene_layout.h, deviceNodes): lo.x hi.x lo.y lo.z | hi.y hi.z skip word */
inline float nodeFloat(const uint32_t* nodes, uint32_t i, int w)
{
    float f;
    memcpy(&f, nodes + 8 * size_t(i) + w, 4);
    return f;
}
inline void nodeBox(const uint32_t* nodes, uint32_t i, float lo[3], float hi[3])
{
    lo[0] = nodeFloat(nodes, i, 0);
    hi[0] = nodeFloat(nodes, i, 1);
    lo[1] = nodeFloat(nodes, i, 2);
    lo[2] = nodeFloat(nodes, i, 3);
    hi[1] = nodeFloat(nodes, i, 4);
    hi[2] = nodeFloat(nodes, i, 5);
}
inline uint32_t nodeSkip(const uint32_t* nodes, uint32_t i) { return nodes[8 * size_t(i) + 6]; }
inline uint32_t nodeWord(const uint32_t* nodes, uint32_t i) { return nodes[8 * size_t(i) + 7]; }
/* an inner node with two children (an empty node has the inner form too: its child link is its own skip link) */
inline bool realInner(const uint32_t* nodes, uint32_t nodeCount, uint32_t i)
{
    const uint32_t word = nodeWord(nodes, i), child = word & NODE_INDEX_MASK;
    return word >= NODE_CHILD && child < nodeCount && child != nodeSkip(nodes, i) && nodeSkip(nodes, child) < nodeCount;
}
inline uint32_t firstChild(const uint32_t* nodes, uint32_t i) { return nodeWord(nodes, i) & NODE_INDEX_MASK; }
inline uint32_t secondChild(const uint32_t* nodes, uint32_t i) { return nodeSkip(nodes, firstChild(nodes, i)); }

/* May node i be left out?  Inner, its six bounds and those of both children numbers, lo <= hi on every axis of all three
 * boxes, and each child's box within its own by float comparison (a tree handed in through the C ABI need not be nested: such
 * nodes stay in the walk).  lo <= hi matters because the box test is symmetric in a slab's two bounds: a box with lo > hi
 * acts as the box with the bounds swapped, which the comparisons of the bounds as stored would take for nested. */
inline bool eligible(const uint32_t* nodes, uint32_t nodeCount, uint32_t i)
{
    if (!realInner(nodes, nodeCount, i))
        return false;
    float lo[3], hi[3];
    nodeBox(nodes, i, lo, hi);
    const uint32_t kids[2] = { firstChild(nodes, i), secondChild(nodes, i) };
    for (int a = 0; a < 3; a++)
        if (!(lo[a] <= hi[a])) /* false for a NaN bound too */
            return false;
    for (uint32_t c : kids) {
        float clo[3], chi[3];
        nodeBox(nodes, c, clo, chi);
        for (int a = 0; a < 3; a++)
            if (!(clo[a] >= lo[a] && chi[a] <= hi[a] && clo[a] <= chi[a])) /* false for a NaN bound of the child's too */
                return false;
    }
    return true;
}

/* ---- the cost model ---- */

/* per node: tests of the reference's walk over the sample that passed and that failed */
struct Counts {
    std::vector<uint64_t> pass, fail;
};

struct Rng { /* splitmix64: the sample is the same on every machine */
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double unit() { return double(next() >> 11) * (1.0 / 9007199254740992.0); }
};

inline bool slabTest(const float lo[3], const float hi[3], const float o[3], const float inv[3], float amin, float amax)
{
    float tmin = amin, tmax = amax;
    for (int a = 0; a < 3; a++) {
        const float t0 = (lo[a] - o[a]) * inv[a], t1 = (hi[a] - o[a]) * inv[a];
        tmin = std::fmax(tmin, std::fmin(t0, t1));
        tmax = std::fmin(tmax, std::fmax(t0, t1));
    }
    return tmin <= tmax;
}

/* the model's triangle test (Moeller-Trumbore in double: it only moves the model's bound, no frame depends on it) */
inline bool modelTriangle(const wpt_tri_geom& t, const float o[3], const float d[3], float amin, float amax, float* a)
{
    double e1[3], e2[3], p[3], s[3], q[3];
    for (int k = 0; k < 3; k++) {
        e1[k] = double(t.v1[k]) - t.v0[k];
        e2[k] = double(t.v2[k]) - t.v0[k];
        s[k] = double(o[k]) - t.v0[k];
    }
    p[0] = d[1] * e2[2] - d[2] * e2[1];
    p[1] = d[2] * e2[0] - d[0] * e2[2];
    p[2] = d[0] * e2[1] - d[1] * e2[0];
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (!(std::fabs(det) > 1e-300))
        return false;
    const double u = (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]) / det;
    q[0] = s[1] * e1[2] - s[2] * e1[1];
    q[1] = s[2] * e1[0] - s[0] * e1[2];
    q[2] = s[0] * e1[1] - s[1] * e1[0];
    const double v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) / det;
    const double w = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
    if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0 && w > double(amin) && w < double(amax)))
        return false;
    *a = float(w);
    return true;
}

/* The sample walks the tree as the reference does (every node, no fold): origins on the triangles (chosen by area), directions
 * uniform in the half-space of the face, a pair of rays per point.  tris: the triangles in the order the nodes' leaf words index.
 * Rays whose slab distances may be NaN are not part of the model (they walk the exact links). */
struct SampleRay {
    float o[3], d[3];
};
/* the amin of every sample ray */
constexpr float SAMPLE_AMIN = 1e-4f;

/* rays (or NULL): the rays that were counted (tests walk them over the link words and count the box tests themselves) */
inline Counts sampleCounts(const uint32_t* nodes, uint32_t nodeCount, const wpt_tri_geom* tris, uint32_t triCount, std::vector<SampleRay>* rays = nullptr)
{
    Counts c;
    c.pass.assign(nodeCount, 0);
    c.fail.assign(nodeCount, 0);
    if (triCount == 0 || !tris)
        return c;
    /* the triangles in the order of their leaves in the tree, depth-first from the root: the sample then is the same whatever
     * order the records are stored in (wpt_scene_upload permutes them, wpt_bypass_plan takes them as given) */
    std::vector<uint32_t> order;
    for (uint32_t node = 0, steps = 0; node < nodeCount && steps < 2 * nodeCount + 2; steps++) {
        const uint32_t word = nodeWord(nodes, node);
        if (word < PRIM_SPHERE_BIT && word < triCount)
            order.push_back(word);
        node = word >= NODE_CHILD ? (word & NODE_INDEX_MASK) : nodeSkip(nodes, node);
    }
    if (order.empty())
        return c;
    std::vector<double> cumulative(order.size());
    double total = 0.0;
    for (size_t i = 0; i < order.size(); i++) {
        double e1[3], e2[3];
        for (int k = 0; k < 3; k++) {
            e1[k] = double(tris[order[i]].v1[k]) - tris[order[i]].v0[k];
            e2[k] = double(tris[order[i]].v2[k]) - tris[order[i]].v0[k];
        }
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double area = std::sqrt(nx * nx + ny * ny + nz * nz);
        total += (area == area && area < 1e300) ? area : 0.0;
        cumulative[i] = total;
    }
    if (!(total > 0.0))
        return c;
    Rng rng = { 0x77757262ull };
    const float amin = SAMPLE_AMIN;
    /* one ray's walk: the nodes tested with their answers; true if the ray hit a triangle */
    std::vector<uint32_t> trace[2];
    auto walk = [&](const float o[3], const float d[3], std::vector<uint32_t>& tested) -> bool {
        tested.clear();
        float inv[3];
        for (int k = 0; k < 3; k++) {
            inv[k] = 1.0f / d[k];
            if (!(std::fabs(inv[k]) < INFINITY) || inv[k] == 0.0f || !(std::fabs(o[k]) < INFINITY))
                return false; /* rayMayNan: not part of the model */
        }
        float amax = INFINITY;
        uint32_t node = 0;
        /* (a depth-first tree ends the walk by itself; the bound is for a tree that is none) */
        for (uint32_t steps = 0; node < nodeCount && steps < 2 * nodeCount + 2; steps++) {
            float blo[3], bhi[3];
            nodeBox(nodes, node, blo, bhi);
            const uint32_t word = nodeWord(nodes, node), skip = nodeSkip(nodes, node);
            const bool hit = slabTest(blo, bhi, o, inv, amin, amax);
            tested.push_back(node << 1 | (hit ? 1u : 0u));
            if (hit && word >= NODE_CHILD) {
                node = word & NODE_INDEX_MASK;
                continue;
            }
            float a;
            if (hit && word < PRIM_SPHERE_BIT && word < triCount && modelTriangle(tris[word], o, d, amin, amax, &a))
                amax = a;
            node = skip;
        }
        return amax < INFINITY;
    };
    for (uint32_t r = 0; r < SAMPLE_RAYS / 2; r++) {
        const double pick = rng.unit() * total;
        uint32_t lo = 0, hi = uint32_t(order.size()) - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (cumulative[mid] > pick)
                hi = mid;
            else
                lo = mid + 1;
        }
        const wpt_tri_geom& t = tris[order[lo]];
        double b0 = rng.unit(), b1 = rng.unit();
        if (b0 + b1 > 1.0) {
            b0 = 1.0 - b0;
            b1 = 1.0 - b1;
        }
        const double z = rng.unit(), phi = 6.283185307179586 * rng.unit();
        double e1[3], e2[3], n[3];
        float o[3], d[2][3];
        for (int k = 0; k < 3; k++) {
            e1[k] = double(t.v1[k]) - t.v0[k];
            e2[k] = double(t.v2[k]) - t.v0[k];
            o[k] = float(t.v0[k] + b0 * e1[k] + b1 * e2[k]);
        }
        n[0] = e1[1] * e2[2] - e1[2] * e2[1];
        n[1] = e1[2] * e2[0] - e1[0] * e2[2];
        n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), el = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        if (!(nl > 0.0) || !(el > 0.0))
            continue;
        double u[3], w[3];
        for (int k = 0; k < 3; k++) {
            n[k] /= nl;
            u[k] = e1[k] / el;
        }
        w[0] = n[1] * u[2] - n[2] * u[1];
        w[1] = n[2] * u[0] - n[0] * u[2];
        w[2] = n[0] * u[1] - n[1] * u[0];
        const double rad = std::sqrt(1.0 - z * z);
        for (int k = 0; k < 3; k++) {
            d[0][k] = float(rad * std::cos(phi) * u[k] + rad * std::sin(phi) * w[k] + z * n[k]);
            d[1][k] = -d[0][k];
        }
        /* a pair of rays from one point, one into either half-space.  Where one of them meets the scene and the other leaves
         * it without a hit, the face is taken for one that encloses the scene (a room's wall seen from inside), and the ray
         * from its back is not one that light takes: it is not counted. */
        const bool met[2] = { walk(o, d[0], trace[0]), walk(o, d[1], trace[1]) };
        for (int side = 0; side < 2; side++) {
            if (!met[side] && met[1 - side])
                continue;
            for (uint32_t v : trace[side])
                ((v & 1u) ? c.pass : c.fail)[v >> 1] += 1;
            if (rays && !trace[side].empty()) {
                SampleRay ray;
                memcpy(ray.o, o, sizeof(ray.o));
                memcpy(ray.d, d[side], sizeof(ray.d));
                rays->push_back(ray);
            }
        }
    }
    return c;
}

/* Box tests of the sample under the walk that folds (wpt_fold.h) and leaves the nodes of `out` alone: a tested node costs its
 * visits; a node that is left out costs, for every visit that would have failed, the tests of its nearest tested descendants
 * (its frontier).  A first child in the fold chain of a tested node is not tested and never fails (its test repeats the
 * chain's head's); the second child starts no chain unless the first is an empty node the fold passes by.  (Not modelled: a
 * tested empty node whose skip link leads to an inner node with its own box, a step the fold takes as well; the model counts
 * those few visits, in the fold's total and the plan's alike.) */
struct Visits {
    const uint32_t* nodes;
    uint32_t nodeCount;
    const Counts* counts;
    const uint8_t* out;
    uint64_t total;
    static constexpr uint32_t NONE = 0xffffffffu;

    /* returns the node's frontier; head: the tested node whose fold chain reaches this first child, or NONE */
    uint64_t at(uint32_t n, uint32_t head, uint32_t depth)
    {
        const uint32_t word = nodeWord(nodes, n);
        const bool folded = head != NONE && word >= NODE_CHILD
                && wptf::foldSameBox(nodes + 8 * size_t(head), nodes + 8 * size_t(n));
        const bool inner = realInner(nodes, nodeCount, n);
        const bool left = inner && out[n] != 0;
        const bool tested = !folded && !left;
        if (tested)
            total += counts->pass[n] + counts->fail[n];
        if (!inner || depth > nodeCount)
            return tested ? 1u : 0u;
        /* (the fold passes an empty first child with the head's box by as well, to the second child, which then is the
         * next node tested: still in the chain) */
        const uint32_t first = firstChild(nodes, n), chain = folded ? head : (tested ? n : NONE);
        const bool emptyFolded = chain != NONE && !realInner(nodes, nodeCount, first) && nodeWord(nodes, first) >= NODE_CHILD
                && wptf::foldSameBox(nodes + 8 * size_t(chain), nodes + 8 * size_t(first));
        const uint64_t frontier = at(first, chain, depth + 1) + at(secondChild(nodes, n), emptyFolded ? chain : NONE, depth + 1);
        if (tested)
            return 1u;
        if (!folded)
            total += counts->fail[n] * frontier;
        return frontier;
    }
};

inline uint64_t visits(const uint32_t* nodes, uint32_t nodeCount, const Counts& counts, const std::vector<uint8_t>& out)
{
    Visits v = { nodes, nodeCount, &counts, out.data(), 0 };
    if (nodeCount > 0)
        v.at(0, Visits::NONE, 0);
    return v.total;
}

/* ---- the plan ---- */

struct Plan {
    /* link words, two per node (skip link, word 7 of the LDS copy: where a ray that passes the box goes, or a leaf's word
     * complemented), links that leave the tree clamped to nodeCount; then the null node's pair (nodeCount, nodeCount); then
     * (the node a ray starts at, 0).  plain: every node's own first child; folded: wpt_fold.h; bypass: folded, with every link
     * that leads to a node of `out` led on to its first child. */
    std::vector<uint32_t> plain, folded, bypass;
    std::vector<uint8_t> out;  /* per node: 1 = left out of the walk */
    uint32_t outCount;
    uint64_t visitsFolded, visitsBypass; /* box tests of the model's sample under the folded links and under the plan's */
};

inline std::vector<uint32_t> linkWords(const uint32_t* nodes, uint32_t nodeCount, bool fold, const std::vector<uint8_t>* out)
{
    auto resolve = [&](uint32_t t) {
        /* (the bound ends a chain that a malformed tree closes to a ring) */
        for (uint32_t k = 0; out && t < nodeCount && (*out)[t] && k < nodeCount; k++)
            t = firstChild(nodes, t);
        return t < nodeCount ? t : nodeCount;
    };
    std::vector<uint32_t> w(2 * size_t(nodeCount) + 4);
    for (uint32_t i = 0; i < nodeCount; i++) {
        uint32_t links;
        const uint32_t word = wptf::foldLdsWord(nodes, nodeCount, i, fold, &links);
        w[2 * size_t(i)] = resolve(nodeSkip(nodes, i));
        w[2 * size_t(i) + 1] = (word & 0x80000000u) ? word : resolve(word);
    }
    w[2 * size_t(nodeCount)] = nodeCount;
    w[2 * size_t(nodeCount) + 1] = nodeCount;
    w[2 * size_t(nodeCount) + 2] = resolve(0);
    w[2 * size_t(nodeCount) + 3] = 0;
    return w;
}

/* nodes: the device nodes of a tree (eight words each); tris: the triangles its leaf words index.  mode: MODE_MODEL or
 * MODE_ALL_ELIGIBLE (tests: every eligible node is left out, whatever it costs). */
inline Plan plan(const uint32_t* nodes, uint32_t nodeCount, const wpt_tri_geom* tris, uint32_t triCount, uint32_t mode)
{
    Plan p;
    p.out.assign(nodeCount, 0);
    p.outCount = 0;
    p.plain = linkWords(nodes, nodeCount, false, nullptr);
    p.folded = linkWords(nodes, nodeCount, true, nullptr);
    std::vector<uint32_t> candidates;
    for (uint32_t i = 0; i < nodeCount; i++)
        if (eligible(nodes, nodeCount, i))
            candidates.push_back(i);
    const Counts counts = sampleCounts(nodes, nodeCount, tris, triCount);
    p.visitsFolded = visits(nodes, nodeCount, counts, p.out);
    uint64_t best = p.visitsFolded;
    if (mode == MODE_ALL_ELIGIBLE) {
        for (uint32_t i : candidates)
            p.out[i] = 1;
        best = visits(nodes, nodeCount, counts, p.out);
    } else {
        /* children before their parents (a first child has the higher index in every storage order deviceNodes makes of a
         * tree this small), again while a pass still finds a node whose absence lowers the sample's visits */
        for (uint32_t pass = 0; pass < SEARCH_PASSES_MAX; pass++) {
            bool changed = false;
            for (size_t k = candidates.size(); k-- > 0;) {
                const uint32_t i = candidates[k];
                if (p.out[i])
                    continue;
                /* the node together with the eligible first children that repeat its box: while the node is tested the fold
                 * passes those by, so they only count once it is gone, and leaving it out alone gains nothing */
                const std::vector<uint8_t> before = p.out;
                p.out[i] = 1;
                for (uint32_t c = firstChild(nodes, i), k2 = 0; k2 < nodeCount && !p.out[c] && eligible(nodes, nodeCount, c)
                        && wptf::foldSameBox(nodes + 8 * size_t(i), nodes + 8 * size_t(c)); c = firstChild(nodes, c), k2++)
                    p.out[c] = 1;
                const uint64_t with = visits(nodes, nodeCount, counts, p.out);
                if (with < best) {
                    best = with;
                    changed = true;
                } else {
                    p.out = before;
                }
            }
            if (!changed)
                break;
        }
    }
    p.visitsBypass = best;
    for (uint32_t i = 0; i < nodeCount; i++)
        p.outCount += p.out[i];
    p.bypass = linkWords(nodes, nodeCount, true, &p.out);
    return p;
}

} // namespace wptb

#endif
