// Harness of tests/test_bypass_walk.py: wptb::eligible, wptb::linkWords and wptb::plan (wurblpt_amd/csrc/wpt_bypass.h), the rule by
// which the walk of a tree in LDS leaves inner nodes out -- the code wpt_scene_upload runs.  Random depth-first trees of up to 200
// nodes with a triangle per leaf: most boxes lie within their parent's by construction (many share planes with it, some repeat
// it bit for bit, which the fold takes), a share has a child box that pokes out of its parent's (by an ulp or by a lot) or has
// lo > hi on an axis (the box test takes it for the box with the bounds swapped, which may reach far outside), every
// tenth tree has a NaN bound, some nodes are empty.  The box test is the kernels' slab arithmetic (wpt_device.h, boxTest), with
// the comparison chains where a slab distance is NaN; rays include directions with zero components (both signs of zero) whose
// origins lie on slab planes of the tree, so that distances are 0 * inf.  A leaf test accepts or not as a function of (leaf, ray,
// bound) and moves the bound: down, or up by an ulp.
// Per tree the reference's walk (every node, over the device words) is set against walks over the link words of four kinds of
// plan: the cost model's, every eligible node, and two random subsets of the eligible nodes.  As in the kernels a ray for which
// rayMayNan holds keeps the folded links, every ray of a tree with a NaN bound does, and the others walk the plan's links -- and
// once more switching between the two sets from step to step, as lanes in a group with a NaN ray do.  Asserted per walk: the
// same leaves under the same bounds in the same order; the nodes the plan's walk does not test are nodes left out or first
// children with their parent's box; the nodes only it tests all fail, below a node left out: so the visits saved are the visits
// to nodes left out minus the extra failing tests.  The cost model's plan has no more visits on its own sample than the fold,
// and the model's closed form is the number of box tests counted when that sample is walked over the folded and the plan's link
// words.  The plan does not depend on the order the triangle records are stored in.  The plan of a tree that fills LDS is timed.
// Two wrong rules must be caught: leaving out inner nodes whatever their children's boxes, and taking a leaf's box for passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_bypass.h"

using namespace wptb;

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
};

enum { INNER, LEAF, EMPTY };
struct Node { float lo[3], hi[3]; int kind; uint32_t second, prim; };

struct Gen {
    Lcg rng;
    std::vector<Node> nodes;
    std::vector<wpt_tri_geom> tris;
    unsigned long long poked = 0, repeated = 0, inverted = 0;
    uint32_t make(int budget, const Node* parent)
    {
        const uint32_t i = (uint32_t)nodes.size();
        nodes.push_back(Node());
        Node nd = Node();
        if (!parent) {
            for (int a = 0; a < 3; a++) {
                nd.lo[a] = (float)(-0.5 * rng.unit());
                nd.hi[a] = (float)(1.0 + 0.5 * rng.unit());
            }
        } else if (rng.unit() < 0.15) {
            memcpy(nd.lo, parent->lo, 12); /* the parent's box bit for bit */
            memcpy(nd.hi, parent->hi, 12);
            repeated++;
        } else {
            for (int a = 0; a < 3; a++) {
                const float w = parent->hi[a] - parent->lo[a];
                float lo = rng.unit() < 0.4 ? parent->lo[a] : parent->lo[a] + (float)(0.6 * rng.unit()) * w;
                float hi = rng.unit() < 0.4 ? parent->hi[a] : parent->hi[a] - (float)(0.6 * rng.unit()) * w;
                if (lo < parent->lo[a]) lo = parent->lo[a];
                if (hi > parent->hi[a]) hi = parent->hi[a];
                if (hi < lo) hi = lo; /* a flat box */
                nd.lo[a] = lo;
                nd.hi[a] = hi;
            }
            if (rng.unit() < 0.08) { /* a bound outside the parent's: by an ulp, or by a lot */
                const int a = (int)(rng.next() % 3u);
                const bool ulp = rng.unit() < 0.5;
                if (rng.unit() < 0.5)
                    nd.hi[a] = ulp ? nextafterf(parent->hi[a], INFINITY) : parent->hi[a] + (float)rng.unit();
                else
                    nd.lo[a] = ulp ? nextafterf(parent->lo[a], -INFINITY) : parent->lo[a] - (float)rng.unit();
                poked++;
            }
            if (rng.unit() < 0.04) { /* lo > hi on an axis: the box test takes such a box for the one with the bounds swapped */
                const int a = (int)(rng.next() % 3u);
                const float lo = nd.lo[a];
                nd.lo[a] = rng.unit() < 0.5 ? nd.hi[a] : parent->hi[a] - (float)rng.unit();
                nd.hi[a] = rng.unit() < 0.5 ? lo : parent->lo[a] - (float)(3.0 * rng.unit());
                if (nd.lo[a] > nd.hi[a])
                    inverted++;
            }
        }
        const bool inner = budget >= 3 && rng.unit() < 0.8;
        if (inner) {
            nd.kind = INNER;
            const int b1 = 1 + (int)(rng.next() % (uint32_t)(budget - 2));
            nodes[i] = nd;
            make(b1, &nd);
            nd.second = make(budget - 1 - b1, &nd);
        } else if (rng.unit() < 0.05) {
            nd.kind = EMPTY;
        } else {
            nd.kind = LEAF;
            nd.prim = (uint32_t)tris.size();
            wpt_tri_geom t = wpt_tri_geom();
            float* v[3] = { t.v0, t.v1, t.v2 };
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++)
                    v[k][a] = nd.lo[a] + (float)rng.unit() * (nd.hi[a] - nd.lo[a]);
            tris.push_back(t);
        }
        nodes[i] = nd;
        return i;
    }
};

struct Ray { float o[3], d[3], inv[3]; bool mayNan; uint32_t id; };

// wpt_device.h, boxTest<CHECK> and boxTestChains, on the host
static bool boxTest(const float* lo, const float* hi, const Ray& r, float amin, float amax, bool check)
{
    float t0[3], t1[3];
    for (int a = 0; a < 3; a++) {
        t0[a] = (lo[a] - r.o[a]) * r.inv[a];
        t1[a] = (hi[a] - r.o[a]) * r.inv[a];
    }
    const float tmin = fmaxf(fmaxf(fminf(t0[0], t1[0]), fminf(t0[1], t1[1])), fmaxf(fminf(t0[2], t1[2]), amin));
    const float tmax = fminf(fminf(fmaxf(t0[0], t1[0]), fmaxf(t0[1], t1[1])), fminf(fmaxf(t0[2], t1[2]), amax));
    bool hit = tmin <= tmax;
    if (check && (t0[0] != t0[0] || t1[0] != t1[0] || t0[1] != t0[1] || t1[1] != t1[1] || t0[2] != t0[2] || t1[2] != t1[2])) {
        float mn[3], mx[3];
        for (int a = 0; a < 3; a++) { /* fminr / fmaxr: (a < b) ? a : b and (a > b) ? a : b */
            mn[a] = t0[a] < t1[a] ? t0[a] : t1[a];
            mx[a] = t0[a] > t1[a] ? t0[a] : t1[a];
        }
        float lo2 = amin, hi2 = amax;
        for (int a = 0; a < 3; a++) {
            if (mn[a] > lo2) lo2 = mn[a];
            if (mx[a] < hi2) hi2 = mx[a];
        }
        hit = lo2 <= hi2;
    }
    return hit;
}

// a leaf test: accepted or not, and the bound it leaves, as a function of (leaf, ray, bound)
static bool leafTest(uint32_t prim, uint32_t ray, float& amax)
{
    uint32_t bits;
    memcpy(&bits, &amax, 4);
    uint64_t h = 1469598103934665603ull;
    h = (h ^ prim) * 1099511628211ull;
    h = (h ^ ray) * 1099511628211ull;
    h = (h ^ bits) * 1099511628211ull;
    h ^= h >> 29;
    h *= 0x9e3779b97f4a7c15ull;
    const uint32_t u = (uint32_t)(h >> 40) % 1000u;
    if (u >= 500)
        return false;
    if (amax > 1e30f)
        amax = 0.05f + 3.0f * (float)(u + 1) / 500.0f;
    else if (u < 40)
        amax = nextafterf(amax, INFINITY); /* accepted by one comparison, stored by another: up by an ulp */
    else
        amax = amax * (0.3f + 0.7f * (float)u / 500.0f);
    return true;
}

// The largest tree the kernels keep in LDS that still has something to sample: 577 nodes and 40 triangles fill the 20 KiB (32 B a
// node, 48 B a triangle); every inner node is eligible and most leaves are empty, the worst case for the search.  Device words.
struct Big {
    std::vector<uint32_t> w;
    std::vector<wpt_tri_geom> tris;
    uint32_t leaves = 0;
    uint32_t make(uint32_t count, const float lo[3], const float hi[3], int axis)
    {
        const uint32_t i = (uint32_t)(w.size() / 8);
        w.resize(w.size() + 8);
        const float box[6] = { lo[0], hi[0], lo[1], lo[2], hi[1], hi[2] };
        if (count == 1) {
            const uint32_t skip = i + 1;
            uint32_t word = NODE_CHILD | skip; /* an empty node */
            if (leaves++ % 7u == 0 && tris.size() < 40) {
                wpt_tri_geom t = wpt_tri_geom();
                for (int a = 0; a < 3; a++) {
                    t.v0[a] = lo[a];
                    t.v1[a] = a == axis ? hi[a] : lo[a];
                    t.v2[a] = hi[a];
                }
                word = (uint32_t)tris.size();
                tris.push_back(t);
            }
            memcpy(&w[8 * (size_t)i], box, 24);
            w[8 * (size_t)i + 6] = skip;
            w[8 * (size_t)i + 7] = word;
            return skip;
        }
        float mid[3] = { hi[0], hi[1], hi[2] }, from[3] = { lo[0], lo[1], lo[2] };
        mid[axis] = from[axis] = 0.5f * (lo[axis] + hi[axis]);
        make(count / 2, lo, mid, (axis + 1) % 3);
        const uint32_t end = make(count - count / 2, from, hi, (axis + 1) % 3);
        memcpy(&w[8 * (size_t)i], box, 24);
        w[8 * (size_t)i + 6] = end;
        w[8 * (size_t)i + 7] = NODE_CHILD | (i + 1);
        return end;
    }
};

struct Step { uint32_t prim, boundBits; };
struct Walk {
    std::vector<Step> leaves;
    std::vector<uint8_t> tested, passed;
    unsigned long long visits = 0;
    bool ended = true;
};

int main()
{
    unsigned long long trees = 0, walks = 0, bad = 0, visitsRef = 0, visitsPlan[4] = { 0, 0, 0, 0 }, extraFailing = 0, leftOutVisits = 0;
    unsigned long long nanRays = 0, nanDistances = 0, nanTrees = 0, poked = 0, inverted = 0, repeated = 0, grown = 0, modelMiscounts = 0, modelRays = 0, modelSkipped = 0, ineligibleInner = 0, eligibleInner = 0;
    unsigned long long caughtIneligible = 0, caughtLeafBox = 0, modelWorse = 0, leftOutModel = 0, nanNodesLeftOut = 0;
    const float amin = 1e-4f;
    for (int t = 0; t < 3000; t++) {
        Gen g;
        g.rng.s = 0xb7a55ull + 104729ull * (uint64_t)t;
        const int budget = 1 + (int)(g.rng.next() % 200u);
        g.make(budget, nullptr);
        const uint32_t n = (uint32_t)g.nodes.size();
        if (n > 200) {
            printf("tree %d has %u nodes\n", t, n);
            return 2;
        }
        bool nanTree = false;
        if (t % 10 == 9) {
            Node& nd = g.nodes[g.rng.next() % n];
            (g.rng.unit() < 0.5 ? nd.lo : nd.hi)[g.rng.next() % 3u] = NAN;
            nanTree = true;
            nanTrees++;
        }
        poked += g.poked;
        inverted += g.inverted;
        repeated += g.repeated;
        /* the device words, as wpt_scene_layout.h makes them */
        std::vector<uint32_t> end(n), parent(n, 0xffffffffu), w(8 * (size_t)n);
        for (uint32_t i = n; i-- > 0;)
            end[i] = g.nodes[i].kind == INNER ? end[g.nodes[i].second] : i + 1;
        for (uint32_t i = 0; i < n; i++) {
            const Node& nd = g.nodes[i];
            const float box[6] = { nd.lo[0], nd.hi[0], nd.lo[1], nd.lo[2], nd.hi[1], nd.hi[2] };
            memcpy(&w[8 * (size_t)i], box, 24);
            w[8 * (size_t)i + 6] = end[i];
            w[8 * (size_t)i + 7] = nd.kind == INNER ? (NODE_CHILD | (i + 1)) : nd.kind == LEAF ? nd.prim : (NODE_CHILD | end[i]);
            if (nd.kind == INNER) {
                parent[i + 1] = i;
                parent[nd.second] = i;
            }
        }
        trees++;
        /* nested, by this file's own comparison */
        std::vector<uint8_t> nested(n, 0), numbers(n, 1);
        for (uint32_t i = 0; i < n; i++)
            for (int a = 0; a < 3; a++)
                if (g.nodes[i].lo[a] != g.nodes[i].lo[a] || g.nodes[i].hi[a] != g.nodes[i].hi[a])
                    numbers[i] = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (g.nodes[i].kind != INNER)
                continue;
            /* by the boxes the test sees: a slab's bounds in either order (a box with lo > hi stays in the walk even where its
             * slabs, taken as intervals, lie within the parent's: the rule asks for lo <= hi) */
            bool ok = numbers[i] && numbers[i + 1] && numbers[g.nodes[i].second];
            for (uint32_t c : { i, i + 1, g.nodes[i].second })
                for (int a = 0; a < 3; a++)
                    ok = ok && g.nodes[c].lo[a] <= g.nodes[c].hi[a] && fminf(g.nodes[c].lo[a], g.nodes[c].hi[a]) >= fminf(g.nodes[i].lo[a], g.nodes[i].hi[a])
                            && fmaxf(g.nodes[c].lo[a], g.nodes[c].hi[a]) <= fmaxf(g.nodes[i].lo[a], g.nodes[i].hi[a]);
            nested[i] = ok;
            (ok ? eligibleInner : ineligibleInner) += 1;
            if (eligible(w.data(), n, i) != ok) {
                printf("tree %d node %u: eligible() says %d\n", t, i, (int)eligible(w.data(), n, i));
                bad++;
            }
        }
        for (uint32_t i = 0; i < n; i++)
            if (g.nodes[i].kind != INNER && eligible(w.data(), n, i))
                bad++;
        /* the plans: 0 the model's, 1 every eligible node, 2 and 3 random subsets; 4: a wrong rule, inner nodes whatever their boxes */
        std::vector<std::vector<uint8_t>> outs(5, std::vector<uint8_t>(n, 0));
        const Plan model = plan(w.data(), n, g.tris.data(), (uint32_t)g.tris.size(), MODE_MODEL);
        const Plan all = plan(w.data(), n, g.tris.data(), (uint32_t)g.tris.size(), MODE_ALL_ELIGIBLE);
        if (t % 8 == 0) { /* same tree, same plan */
            const Plan again = plan(w.data(), n, g.tris.data(), (uint32_t)g.tris.size(), MODE_MODEL);
            if (again.bypass != model.bypass || again.out != model.out)
                bad++;
            /* ... whatever order its triangle records are stored in (wpt_scene_upload stores them in the order of their leaves) */
            const uint32_t m = (uint32_t)g.tris.size();
            std::vector<uint32_t> w2(w);
            std::vector<wpt_tri_geom> tris2(m);
            for (uint32_t i = 0; i < n; i++)
                if (g.nodes[i].kind == LEAF)
                    w2[8 * (size_t)i + 7] = m - 1 - g.nodes[i].prim;
            for (uint32_t k = 0; k < m; k++)
                tris2[m - 1 - k] = g.tris[k];
            if (plan(w2.data(), n, tris2.data(), m, MODE_MODEL).out != model.out)
                bad++;
        }
        if (model.visitsBypass > model.visitsFolded)
            modelWorse++;
        /* (one case the closed form leaves out, and counts a few visits too many in: a tested empty node whose skip link leads
         * to an inner node with the empty node's own box -- the fold takes that step too) */
        bool emptyOntoSame = false;
        for (uint32_t i = 0; i < n; i++)
            if (g.nodes[i].kind == EMPTY && end[i] < n && w[8 * (size_t)end[i] + 7] >= NODE_CHILD && memcmp(&w[8 * (size_t)i], &w[8 * (size_t)end[i]], 24) == 0)
                emptyOntoSame = true;
        modelSkipped += emptyOntoSame ? 1 : 0;
        if (!nanTree && !emptyOntoSame) {
            /* the model's closed form against box tests counted: its own sample walked over the folded and the plan's link words */
            std::vector<SampleRay> sample;
            sampleCounts(w.data(), n, g.tris.data(), (uint32_t)g.tris.size(), &sample);
            modelRays += sample.size();
            const std::vector<uint32_t>* sets[2] = { &model.folded, &model.bypass };
            unsigned long long counted[2] = { 0, 0 };
            for (int k = 0; k < 2; k++)
                for (const SampleRay& sr : sample) {
                    float inv[3] = { 1.0f / sr.d[0], 1.0f / sr.d[1], 1.0f / sr.d[2] }, amax = INFINITY;
                    uint32_t node = (*sets[k])[2 * (size_t)n + 2];
                    for (uint32_t steps = 0; node < n && steps < 4 * n + 4; steps++) {
                        counted[k]++;
                        const bool hit = slabTest(g.nodes[node].lo, g.nodes[node].hi, sr.o, inv, SAMPLE_AMIN, amax);
                        const uint32_t skip = (*sets[k])[2 * (size_t)node], word = (*sets[k])[2 * (size_t)node + 1];
                        float a;
                        if (hit && (int32_t)word < 0 && modelTriangle(g.tris[~word], sr.o, sr.d, SAMPLE_AMIN, amax, &a))
                            amax = a;
                        node = (hit && (int32_t)word >= 0) ? word : skip;
                    }
                }
            if (counted[0] != model.visitsFolded || counted[1] != model.visitsBypass) {
                if (modelMiscounts < 5)
                    printf("tree %d: the model says %llu / %llu visits, counted %llu / %llu\n", t, (unsigned long long)model.visitsFolded, (unsigned long long)model.visitsBypass, counted[0], counted[1]);
                modelMiscounts++;
            }
        }
        outs[0] = model.out;
        outs[1] = all.out;
        leftOutModel += model.outCount;
        for (uint32_t i = 0; i < n; i++) {
            if (all.out[i] != nested[i])
                bad++;
            if (nested[i]) {
                outs[2][i] = g.rng.unit() < 0.5;
                outs[3][i] = g.rng.unit() < 0.25;
            }
            if (g.nodes[i].kind == INNER && numbers[i])
                outs[4][i] = g.rng.unit() < 0.7;
            for (int k = 0; k < 4; k++)
                if (outs[k][i] && (!nested[i] || !numbers[i]))
                    nanNodesLeftOut++;
        }
        const std::vector<uint32_t> folded = linkWords(w.data(), n, true, nullptr);
        if (folded != model.folded)
            bad++;
        std::vector<std::vector<uint32_t>> links;
        for (int k = 0; k < 5; k++)
            links.push_back(linkWords(w.data(), n, true, &outs[k]));
        if (links[0] != model.bypass)
            bad++;

        for (uint32_t q = 0; q < 16; q++) {
            Ray r;
            r.id = (uint32_t)t * 64u + q;
            for (int a = 0; a < 3; a++) {
                r.o[a] = (float)(-1.0 + 3.0 * g.rng.unit());
                r.d[a] = (float)(g.rng.unit() - 0.5);
            }
            if (q % 2 == 0) /* towards a point of the root's box: walks that go deep */
                for (int a = 0; a < 3; a++)
                    r.d[a] = g.nodes[0].lo[a] + (float)g.rng.unit() * (g.nodes[0].hi[a] - g.nodes[0].lo[a]) - r.o[a];
            if (q % 4 == 3) { /* one or two zero components, of either sign, the origin on a slab plane of the tree */
                const int zeros = 1 + (int)(g.rng.next() % 2u);
                for (int z = 0; z < zeros; z++) {
                    const int a = (int)(g.rng.next() % 3u);
                    r.d[a] = g.rng.unit() < 0.5 ? 0.0f : -0.0f;
                    const Node& nd = g.nodes[g.rng.next() % n];
                    if (g.rng.unit() < 0.7)
                        r.o[a] = g.rng.unit() < 0.5 ? nd.lo[a] : nd.hi[a];
                }
                if (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f)
                    r.d[g.rng.next() % 3u] = 1.0f;
            }
            r.mayNan = false;
            for (int a = 0; a < 3; a++) {
                r.inv[a] = 1.0f / r.d[a];
                if (!(fabsf(r.inv[a]) < INFINITY) || r.inv[a] == 0.0f || !(fabsf(r.o[a]) < INFINITY))
                    r.mayNan = true; /* wpt_device.h, rayMayNan */
            }
            nanRays += r.mayNan ? 1 : 0;
            const bool exactOnly = r.mayNan || nanTree; /* what the kernels do: RAY_MAY_NAN, SceneView::boxesMayBeNan */

            /* the reference's walk: every node, over the device words (binaryStep) */
            Walk ref;
            ref.tested.assign(n, 0);
            ref.passed.assign(n, 0);
            {
                float amax = 3.0e38f;
                uint32_t node = 0;
                while (node < n) {
                    ref.visits++;
                    const Node& nd = g.nodes[node];
                    for (int a = 0; a < 3; a++) {
                        const float d0 = (nd.lo[a] - r.o[a]) * r.inv[a], d1 = (nd.hi[a] - r.o[a]) * r.inv[a];
                        nanDistances += (d0 != d0 || d1 != d1) ? 1 : 0;
                    }
                    const bool hit = boxTest(nd.lo, nd.hi, r, amin, amax, true);
                    ref.tested[node] = 1;
                    ref.passed[node] = hit;
                    const uint32_t word = w[8 * (size_t)node + 7];
                    if (hit && word >= NODE_CHILD) {
                        node = word & NODE_INDEX_MASK;
                    } else {
                        if (hit) {
                            uint32_t bits;
                            memcpy(&bits, &amax, 4);
                            const float before = amax;
                            ref.leaves.push_back({ word, bits });
                            if (leafTest(word, r.id, amax) && amax > before)
                                grown++;
                        }
                        node = w[8 * (size_t)node + 6];
                    }
                }
            }
            visitsRef += ref.visits;

            /* the walk over link words (ldsStep and the leaf test's decoding); mix: the set changes from step to step */
            auto walk = [&](const std::vector<uint32_t>& plain, const std::vector<uint32_t>& exact, bool mix, const std::vector<uint8_t>* leafBoxPassed) {
                Walk k;
                k.tested.assign(n, 0);
                k.passed.assign(n, 0);
                float amax = 3.0e38f;
                Lcg pick = { 0x51ull + r.id };
                const std::vector<uint32_t>* use = exactOnly ? &exact : &plain;
                uint32_t node = (*use)[2 * (size_t)n + 2];
                if (exactOnly && node != 0)
                    bad++;
                while (node < n) {
                    if (!exactOnly && mix)
                        use = (pick.next() & 1u) ? &exact : &plain;
                    k.visits++;
                    if (k.visits > 100000) {
                        k.ended = false;
                        break;
                    }
                    const Node& nd = g.nodes[node];
                    bool hit = boxTest(nd.lo, nd.hi, r, amin, amax, exactOnly);
                    const uint32_t skip = (*use)[2 * (size_t)node], word = (*use)[2 * (size_t)node + 1];
                    if (leafBoxPassed && (*leafBoxPassed)[node])
                        hit = true;
                    k.tested[node] = 1;
                    k.passed[node] = hit;
                    if (hit && (int32_t)word < 0) {
                        uint32_t bits;
                        memcpy(&bits, &amax, 4);
                        k.leaves.push_back({ ~word, bits });
                        leafTest(~word, r.id, amax);
                        node = skip;
                    } else {
                        node = hit ? word : skip;
                    }
                }
                return k;
            };
            auto sameLeaves = [&](const Walk& a, const Walk& b) {
                if (!b.ended || a.leaves.size() != b.leaves.size())
                    return false;
                for (size_t i = 0; i < a.leaves.size(); i++)
                    if (a.leaves[i].prim != b.leaves[i].prim || a.leaves[i].boundBits != b.leaves[i].boundBits)
                        return false;
                return true;
            };
            for (int k = 0; k < 4; k++) {
                const Walk got = walk(links[k], folded, false, nullptr);
                walks++;
                bool ok = sameLeaves(ref, got);
                unsigned long long skipped = 0, extra = 0;
                for (uint32_t i = 0; i < n && ok; i++) {
                    if (ref.tested[i] && !got.tested[i]) {
                        /* left out (rays that keep the exact links: never), or a first child with its parent's box: the fold */
                        const uint32_t p = parent[i];
                        /* (the fold passes an empty first child by as well: then the second child is the next node tested) */
                        const bool foldable = p != 0xffffffffu && (i == p + 1 || g.nodes[p + 1].kind == EMPTY) && w[8 * (size_t)i + 7] >= NODE_CHILD
                                && memcmp(&w[8 * (size_t)i], &w[8 * (size_t)p], 24) == 0;
                        if (outs[k][i] && !exactOnly)
                            skipped++;
                        else if (!foldable)
                            ok = false;
                    } else if (!ref.tested[i] && got.tested[i]) {
                        /* an extra test: it fails, and the node lies below a node that is left out */
                        bool below = false;
                        for (uint32_t p = parent[i]; p != 0xffffffffu; p = parent[p])
                            below = below || outs[k][p];
                        if (got.passed[i] || !below || exactOnly)
                            ok = false;
                        extra++;
                    } else if (ref.tested[i] && ref.passed[i] != got.passed[i]) {
                        ok = false;
                    }
                }
                visitsPlan[k] += got.visits;
                leftOutVisits += skipped;
                extraFailing += extra;
                if (!ok) {
                    if (bad < 10)
                        printf("tree %d plan %d ray %u: %zu / %zu leaves, visits %llu / %llu\n", t, k, q, ref.leaves.size(), got.leaves.size(), ref.visits, got.visits);
                    bad++;
                }
                const Walk mixed = walk(links[k], folded, true, nullptr);
                walks++;
                if (!sameLeaves(ref, mixed)) {
                    if (bad < 10)
                        printf("tree %d plan %d ray %u, mixed links: %zu / %zu leaves\n", t, k, q, ref.leaves.size(), mixed.leaves.size());
                    bad++;
                }
            }
            /* the wrong rules */
            if (!exactOnly) {
                if (!sameLeaves(ref, walk(links[4], folded, false, nullptr)))
                    caughtIneligible++;
                std::vector<uint8_t> leafBoxPassed(n, 0);
                for (uint32_t i = 0; i < n; i++)
                    leafBoxPassed[i] = g.nodes[i].kind == LEAF && g.rng.unit() < 0.5;
                if (!sameLeaves(ref, walk(folded, folded, false, &leafBoxPassed)))
                    caughtLeafBox++;
            }
        }
    }
    {
        Big big;
        const float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
        big.make(289, lo, hi, 0);
        const uint32_t n = (uint32_t)(big.w.size() / 8);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const Plan p = plan(big.w.data(), n, big.tris.data(), (uint32_t)big.tris.size(), MODE_MODEL);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        printf("plan of a tree of %u nodes, %zu triangles (%zu bytes in LDS): %u nodes left out, visits %llu -> %llu, %.1f ms\n", n, big.tris.size(),
                (size_t)n * 32 + big.tris.size() * 48, p.outCount, (unsigned long long)p.visitsFolded, (unsigned long long)p.visitsBypass,
                1e3 * (double)(t1.tv_sec - t0.tv_sec) + 1e-6 * (double)(t1.tv_nsec - t0.tv_nsec));
        if (n != 577 || big.tris.size() != 40 || p.visitsBypass > p.visitsFolded)
            bad++;
    }
    printf("trees %llu, walks %llu, node visits of the reference's walk %llu\n", trees, walks, visitsRef);
    printf("inner nodes: %llu eligible, %llu not; children that poke out %llu, boxes with lo > hi %llu, boxes repeated %llu, trees with a NaN bound %llu\n", eligibleInner, ineligibleInner, poked, inverted, repeated, nanTrees);
    printf("rays with RAY_MAY_NAN %llu, NaN slab distances %llu, bounds grown by an ulp %llu\n", nanRays, nanDistances, grown);
    printf("visits by plan: model %llu, all eligible %llu, subsets %llu %llu; nodes the model leaves out %llu\n", visitsPlan[0], visitsPlan[1], visitsPlan[2], visitsPlan[3], leftOutModel);
    printf("visits to nodes left out %llu, extra failing tests %llu\n", leftOutVisits, extraFailing);
    printf("model plans with more visits on their sample than the fold: %llu\n", modelWorse);
    printf("sample rays walked over the link words %llu; trees whose counted box tests differ from the model's closed form: %llu (%llu trees with an empty node that folds onto its successor not compared)\n", modelRays, modelMiscounts, modelSkipped);
    printf("ineligible nodes left out: %llu\n", nanNodesLeftOut);
    printf("wrong rules caught: inner nodes whatever their boxes %llu, a leaf's box taken for passed %llu\n", caughtIneligible, caughtLeafBox);
    const bool covered = ineligibleInner > 0 && inverted > 0 && modelRays > 0 && poked > 0 && repeated > 0 && nanTrees > 0 && nanRays > 0 && nanDistances > 0 && grown > 0
            && leftOutVisits > 0 && extraFailing > 0 && leftOutModel > 0 && caughtIneligible > 0 && caughtLeafBox > 0;
    printf("cases covered: %s\n", covered ? "yes" : "NO");
    printf("walks that differ: %llu\n", bad);
    return bad == 0 && covered && modelWorse == 0 && modelMiscounts == 0 && nanNodesLeftOut == 0 ? 0 : 1;
}
