// Harness of tests/test_leaf_words.py: wptw::leafWords (wurblpt_amd/csrc/wpt_leaf_words.h), the words that let the leaf pass of
// the kernels with rotated corner copies do without the leaf's node -- the code wpt_scene_upload runs.  Trees: seeded random
// depth-first trees of up to 200 nodes with a triangle per leaf (boxes that repeat their parent's, which the fold takes; empty
// nodes; every tenth tree with a NaN bound), a tree that fills LDS (577 nodes, 40 triangles), and the trees of the files named on
// the command line (the Cornell box's: tests/test_leaf_words.py writes its device words).  Per tree and per set of link words
// of its plan (wpt_bypass.h: plain, folded, bypass):
//   - every leaf's word names its node and its triangle's first corner, the triangle's words are the leaf's skip link under
//     that set, and every other word is the set's own; the verdict is "one to one";
//   - a model of the walk that takes a leaf's triangle and successor from the per-triangle words (the corner records the
//     kernels' prologue writes: skip link under the launch's links, exact skip link, triangle) performs the leaf tests of the
//     model that reads them from the leaf's node (the kernels' leaf pass before): the same triangles under the same bounds in
//     the same order, for rays with and without RAY_MAY_NAN, and with the exact and the launch's links taking turns from one
//     look to the next as they do in a wave whose rays with RAY_MAY_NAN come and go; so does the model of the leaf pass for
//     trees that are not one to one (the node's index from the leaf word, the links from the node).
// Two hand-made trees must get the verdict "not one to one": two leaves that name one triangle, a triangle that no leaf names;
// and a tree whose indices do not fit the word "too large".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_bypass.h"
#include "../wurblpt_amd/csrc/wpt_leaf_words.h"

using namespace wptb;

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
};

struct Tree {
    std::vector<uint32_t> w; /* device words, eight per node */
    std::vector<wpt_tri_geom> tris;
    uint32_t nodes() const { return (uint32_t)(w.size() / 8); }
};

/* a random depth-first tree: returns the first node behind the subtree */
static uint32_t grow(Tree& t, Lcg& rng, int budget, const float* plo, const float* phi)
{
    const uint32_t i = t.nodes();
    t.w.resize(t.w.size() + 8);
    float lo[3], hi[3];
    const bool repeat = plo && rng.unit() < 0.15; /* the parent's box bit for bit */
    for (int a = 0; a < 3; a++) {
        if (!plo) {
            lo[a] = (float)(-0.5 * rng.unit());
            hi[a] = (float)(1.0 + 0.5 * rng.unit());
        } else if (repeat) {
            lo[a] = plo[a];
            hi[a] = phi[a];
        } else {
            const float width = phi[a] - plo[a];
            lo[a] = rng.unit() < 0.4 ? plo[a] : plo[a] + (float)(0.6 * rng.unit()) * width;
            hi[a] = rng.unit() < 0.4 ? phi[a] : phi[a] - (float)(0.6 * rng.unit()) * width;
            if (hi[a] < lo[a])
                hi[a] = lo[a];
            if (rng.unit() < 0.03) /* a bound outside the parent's */
                hi[a] = phi[a] + (float)rng.unit();
        }
    }
    const float box[6] = { lo[0], hi[0], lo[1], lo[2], hi[1], hi[2] };
    uint32_t end, word;
    if (budget >= 3 && rng.unit() < 0.8) {
        const int b1 = 1 + (int)(rng.next() % (uint32_t)(budget - 2));
        grow(t, rng, b1, lo, hi);
        end = grow(t, rng, budget - 1 - b1, lo, hi);
        word = NODE_CHILD | (i + 1);
    } else {
        end = i + 1;
        if (rng.unit() < 0.05) {
            word = NODE_CHILD | end; /* an empty node */
        } else {
            word = (uint32_t)t.tris.size();
            wpt_tri_geom g = wpt_tri_geom();
            float* v[3] = { g.v0, g.v1, g.v2 };
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++)
                    v[k][a] = lo[a] + (float)rng.unit() * (hi[a] - lo[a]);
            t.tris.push_back(g);
        }
    }
    memcpy(&t.w[8 * (size_t)i], box, 24);
    t.w[8 * (size_t)i + 6] = end;
    t.w[8 * (size_t)i + 7] = word;
    return end;
}

/* the largest tree the kernels keep in LDS that still has triangles: halves of the unit cube, every seventh leaf a triangle */
static uint32_t halve(Tree& t, uint32_t& leaves, uint32_t count, const float lo[3], const float hi[3], int axis)
{
    const uint32_t i = t.nodes();
    t.w.resize(t.w.size() + 8);
    const float box[6] = { lo[0], hi[0], lo[1], lo[2], hi[1], hi[2] };
    uint32_t end, word;
    if (count == 1) {
        end = i + 1;
        word = NODE_CHILD | end;
        if (leaves++ % 7u == 0 && t.tris.size() < 40) {
            wpt_tri_geom g = wpt_tri_geom();
            for (int a = 0; a < 3; a++) {
                g.v0[a] = lo[a];
                g.v1[a] = a == axis ? hi[a] : lo[a];
                g.v2[a] = hi[a];
            }
            word = (uint32_t)t.tris.size();
            t.tris.push_back(g);
        }
    } else {
        float mid[3] = { hi[0], hi[1], hi[2] }, from[3] = { lo[0], lo[1], lo[2] };
        mid[axis] = from[axis] = 0.5f * (lo[axis] + hi[axis]);
        halve(t, leaves, count / 2, lo, mid, (axis + 1) % 3);
        end = halve(t, leaves, count - count / 2, from, hi, (axis + 1) % 3);
        word = NODE_CHILD | (i + 1);
    }
    memcpy(&t.w[8 * (size_t)i], box, 24);
    t.w[8 * (size_t)i + 6] = end;
    t.w[8 * (size_t)i + 7] = word;
    return end;
}

/* a file of tests/test_leaf_words.py: node count, triangle count, the device words, the triangle records */
static bool load(const char* path, Tree& t)
{
    FILE* f = fopen(path, "rb");
    if (!f)
        return false;
    uint32_t counts[2] = { 0, 0 };
    bool ok = fread(counts, 4, 2, f) == 2 && counts[0] > 0 && counts[0] < 100000 && counts[1] < 100000;
    if (ok) {
        t.w.resize(8 * (size_t)counts[0]);
        t.tris.resize(counts[1]);
        ok = fread(t.w.data(), 32, counts[0], f) == counts[0] && fread(t.tris.data(), sizeof(wpt_tri_geom), counts[1], f) == counts[1];
    }
    fclose(f);
    return ok;
}

struct Ray { float o[3], d[3], inv[3]; bool mayNan; uint32_t id; };

static void finish(Ray& r)
{
    r.mayNan = false;
    for (int a = 0; a < 3; a++) {
        r.inv[a] = 1.0f / r.d[a];
        if (!(fabsf(r.inv[a]) < INFINITY) || r.inv[a] == 0.0f || !(fabsf(r.o[a]) < INFINITY))
            r.mayNan = true; /* wpt_device.h, rayMayNan */
    }
}

// wpt_device.h, boxTest<CHECK> and boxTestChains, on the host
static bool boxTest(const uint32_t* node, const Ray& r, float amin, float amax, bool check)
{
    float lo[3], hi[3], t0[3], t1[3];
    nodeBox(node, 0, lo, hi);
    for (int a = 0; a < 3; a++) {
        t0[a] = (lo[a] - r.o[a]) * r.inv[a];
        t1[a] = (hi[a] - r.o[a]) * r.inv[a];
    }
    const float tmin = fmaxf(fmaxf(fminf(t0[0], t1[0]), fminf(t0[1], t1[1])), fmaxf(fminf(t0[2], t1[2]), amin));
    const float tmax = fminf(fminf(fmaxf(t0[0], t1[0]), fmaxf(t0[1], t1[1])), fminf(fmaxf(t0[2], t1[2]), amax));
    bool hit = tmin <= tmax;
    if (check && (t0[0] != t0[0] || t1[0] != t1[0] || t0[1] != t0[1] || t1[1] != t1[1] || t0[2] != t0[2] || t1[2] != t1[2])) {
        float lo2 = amin, hi2 = amax;
        for (int a = 0; a < 3; a++) {
            const float mn = t0[a] < t1[a] ? t0[a] : t1[a], mx = t0[a] > t1[a] ? t0[a] : t1[a];
            if (mn > lo2) lo2 = mn;
            if (mx < hi2) hi2 = mx;
        }
        hit = lo2 <= hi2;
    }
    return hit;
}

// a leaf test: accepted or not, and the bound it leaves, as a function of (triangle, ray, bound)
static void leafTest(uint32_t prim, uint32_t ray, float& amax)
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
        return;
    if (amax > 1e30f)
        amax = 0.05f + 3.0f * (float)(u + 1) / 500.0f;
    else if (u < 40)
        amax = nextafterf(amax, INFINITY);
    else
        amax = amax * (0.3f + 0.7f * (float)u / 500.0f);
}

struct Step { uint32_t prim, boundBits; };
enum Form { FROM_NODE, FROM_RECORDS, FROM_WORD_NODE };

struct Counters {
    unsigned long long trees = 0, sets = 0, leaves = 0, walks = 0, leafTests = 0, nanWalks = 0, mixedWalks = 0, wrongWords = 0, wrongVerdicts = 0, differ = 0;
};

/* A ray's walk.  launch / exact: link words of the set the launch walks and of the exact one (FROM_NODE: wpt_bypass.h's; the
 * other forms: leafWords' of the same sets).  nanTree: every look takes the exact links; a ray with RAY_MAY_NAN too; `mixed`:
 * other looks do by the toss of a coin (the same coins in every form). */
static std::vector<Step> walk(const Tree& t, const std::vector<uint32_t>& launch, const std::vector<uint32_t>& exact, Form form, const Ray& r, bool nanTree, bool mixed)
{
    const uint32_t n = t.nodes();
    const size_t tris = wptw::leafWordsTriangles(n);
    std::vector<Step> out;
    float amax = 3.0e38f;
    Lcg coin = { 0x51ull + r.id };
    uint32_t node = (r.mayNan || nanTree) ? 0u : launch[2 * (size_t)n + 2]; /* beginRay: rays with RAY_MAY_NAN start at the root */
    for (uint32_t looks = 0; node < n && looks < 100000; looks++) {
        bool nan = r.mayNan || nanTree;
        if (!nan && mixed)
            nan = (coin.next() & 1u) != 0;
        const std::vector<uint32_t>& use = nan ? exact : launch;
        const bool hit = boxTest(&t.w[8 * (size_t)node], r, 1e-4f, amax, nan);
        const uint32_t skip = use[2 * (size_t)node], word = use[2 * (size_t)node + 1];
        if (!(hit && (int32_t)word < 0)) {
            node = hit ? word : skip;
            continue;
        }
        /* the leaf pass, possibly at a later look: the exact links or not is that look's */
        if (!(r.mayNan || nanTree) && mixed)
            nan = (coin.next() & 1u) != 0;
        uint32_t prim, next;
        if (form == FROM_NODE) {
            /* ldsStep kept the node's index; the LDS copy of the node has the launch's words */
            prim = ~launch[2 * (size_t)node + 1];
            next = nan ? exact[2 * (size_t)node] : launch[2 * (size_t)node];
        } else {
            /* ldsStep kept the word; the records of the triangle at its corner offset (the prologue's copy) */
            const uint32_t corner = wptw::leafWordCorner(word), triangle = corner / 3u;
            const uint32_t record[3] = { launch[tris + triangle], exact[tris + triangle], triangle };
            prim = record[2];
            next = nan ? record[1] : record[0];
            if (form == FROM_WORD_NODE) {
                const uint32_t leaf = wptw::leafWordNode(word);
                next = nan ? exact[2 * (size_t)leaf] : launch[2 * (size_t)leaf];
            }
        }
        uint32_t bits;
        memcpy(&bits, &amax, 4);
        out.push_back({ prim, bits });
        leafTest(prim, r.id, amax);
        node = next;
    }
    return out;
}

static bool same(const std::vector<Step>& a, const std::vector<Step>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].prim != b[i].prim || a[i].boundBits != b[i].boundBits)
            return false;
    return true;
}

/* the checks of one tree; oneToOne: what the verdict must be */
static void check(const Tree& t, bool nanTree, bool oneToOne, uint32_t seed, Counters& c)
{
    const uint32_t n = t.nodes(), m = (uint32_t)t.tris.size();
    const size_t tris = wptw::leafWordsTriangles(n);
    const Plan p = plan(t.w.data(), n, t.tris.data(), m, MODE_MODEL);
    const std::vector<uint32_t>* sets[3] = { &p.plain, &p.folded, &p.bypass };
    std::vector<wptw::LeafWords> leaf;
    c.trees++;
    for (int k = 0; k < 3; k++) {
        const std::vector<uint32_t>& links = *sets[k];
        leaf.push_back(wptw::leafWords(links.data(), n, m));
        const wptw::LeafWords& lw = leaf.back();
        c.sets++;
        if ((lw.verdict == wptw::ONE_TO_ONE) != oneToOne || lw.verdict == wptw::TOO_LARGE)
            c.wrongVerdicts++;
        if (lw.words.size() != wptw::leafWordsSize(n, m) || (lw.words.size() & 1u)) {
            c.wrongWords++;
            continue;
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t word = nodeWord(t.w.data(), i);
            if (lw.words[2 * (size_t)i] != links[2 * (size_t)i])
                c.wrongWords++;
            if (word >= NODE_CHILD) {
                if (lw.words[2 * (size_t)i + 1] != links[2 * (size_t)i + 1])
                    c.wrongWords++;
                continue;
            }
            c.leaves++;
            const uint32_t got = lw.words[2 * (size_t)i + 1];
            if (!(got & wptw::LEAF_BIT) || got != wptw::leafWord(i, word) || wptw::leafWordNode(got) != i || wptw::leafWordCorner(got) != 3 * word)
                c.wrongWords++;
            /* the triangle's words: its leaf's skip link under these links, which for the exact sets is the exact skip link */
            if (oneToOne && lw.words[tris + word] != links[2 * (size_t)i])
                c.wrongWords++;
        }
        for (size_t i = 2 * (size_t)n; i < tris; i++)
            if (lw.words[i] != links[i])
                c.wrongWords++;
    }
    /* rays: the cost model's own sample of the scene, rays from outside, and rays with zero components from slab planes */
    std::vector<Ray> rays;
    std::vector<SampleRay> sample;
    sampleCounts(t.w.data(), n, t.tris.data(), m, &sample);
    Lcg rng = { 0x1eafull + seed };
    for (size_t i = 0; i < sample.size() && rays.size() < 24; i += sample.size() / 24 + 1) {
        Ray r;
        memcpy(r.o, sample[i].o, 12);
        memcpy(r.d, sample[i].d, 12);
        rays.push_back(r);
    }
    float rootLo[3], rootHi[3];
    nodeBox(t.w.data(), 0, rootLo, rootHi);
    for (int q = 0; q < 16; q++) {
        Ray r;
        for (int a = 0; a < 3; a++) {
            r.o[a] = (float)(-1.0 + 3.0 * rng.unit());
            r.d[a] = rootLo[a] + (float)rng.unit() * (rootHi[a] - rootLo[a]) - r.o[a];
            if (r.d[a] != r.d[a]) /* a NaN bound of the root's */
                r.d[a] = 0.25f;
        }
        if (q % 4 == 3) {
            const int zeros = 1 + (int)(rng.next() % 2u);
            for (int z = 0; z < zeros; z++) {
                const int a = (int)(rng.next() % 3u);
                r.d[a] = rng.unit() < 0.5 ? 0.0f : -0.0f;
                float lo[3], hi[3];
                nodeBox(t.w.data(), rng.next() % n, lo, hi);
                if (rng.unit() < 0.7)
                    r.o[a] = rng.unit() < 0.5 ? lo[a] : hi[a];
            }
            if (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f)
                r.d[rng.next() % 3u] = 1.0f;
        }
        rays.push_back(r);
    }
    for (size_t q = 0; q < rays.size(); q++) {
        Ray& r = rays[q];
        r.id = seed * 64u + (uint32_t)q;
        finish(r);
        /* launches: (exact, launch) = (plain, plain) under WPT_WALK_NO_FOLD, (folded, folded) without the bypass, (folded, bypass) */
        const int pairs[3][2] = { { 0, 0 }, { 1, 1 }, { 1, 2 } };
        for (int k = 0; k < 3; k++) {
            const int e = pairs[k][0], l = pairs[k][1];
            for (int mixed = 0; mixed < 2; mixed++) {
                const std::vector<Step> ref = walk(t, *sets[l], *sets[e], FROM_NODE, r, nanTree, mixed != 0);
                const std::vector<Step> fromNode = walk(t, leaf[l].words, leaf[e].words, FROM_WORD_NODE, r, nanTree, mixed != 0);
                c.walks += 2;
                c.leafTests += ref.size();
                c.nanWalks += (r.mayNan || nanTree) ? 1 : 0;
                c.mixedWalks += mixed;
                if (!same(ref, fromNode))
                    c.differ++;
                if (oneToOne) {
                    c.walks++;
                    if (!same(ref, walk(t, leaf[l].words, leaf[e].words, FROM_RECORDS, r, nanTree, mixed != 0)))
                        c.differ++;
                }
            }
        }
    }
}

int main(int argc, char** argv)
{
    Counters c;
    unsigned long long nanTrees = 0, emptyNodes = 0, foldedNodes = 0, bypassedNodes = 0, files = 0;
    for (int t = 0; t < 300; t++) {
        Tree tree;
        Lcg rng = { 0x1ea5ull + 104729ull * (uint64_t)t };
        grow(tree, rng, 1 + (int)(rng.next() % 200u), nullptr, nullptr);
        const uint32_t n = tree.nodes();
        bool nanTree = false;
        if (t % 10 == 9) {
            uint32_t bits;
            const float nan = NAN;
            memcpy(&bits, &nan, 4);
            tree.w[8 * (size_t)(rng.next() % n) + rng.next() % 6u] = bits;
            nanTree = true;
            nanTrees++;
        }
        for (uint32_t i = 0; i < n; i++)
            emptyNodes += nodeWord(tree.w.data(), i) >= NODE_CHILD && !realInner(tree.w.data(), n, i) ? 1 : 0;
        const Plan p = plan(tree.w.data(), n, tree.tris.data(), (uint32_t)tree.tris.size(), MODE_MODEL);
        bypassedNodes += p.outCount;
        for (uint32_t i = 0; i < n; i++)
            foldedNodes += p.folded[2 * (size_t)i + 1] != p.plain[2 * (size_t)i + 1] ? 1 : 0;
        check(tree, nanTree, true, (uint32_t)t, c);
    }
    {
        Tree big;
        uint32_t leaves = 0;
        const float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
        halve(big, leaves, 289, lo, hi, 0);
        if (big.nodes() != 577 || big.tris.size() != 40) {
            printf("the tree that fills LDS has %u nodes, %zu triangles\n", big.nodes(), big.tris.size());
            return 2;
        }
        check(big, false, true, 1000u, c);
    }
    for (int a = 1; a < argc; a++) {
        Tree tree;
        if (!load(argv[a], tree)) {
            printf("cannot read %s\n", argv[a]);
            return 2;
        }
        printf("tree of %s: %u nodes, %zu triangles\n", argv[a], tree.nodes(), tree.tris.size());
        check(tree, false, true, 2000u + (uint32_t)a, c);
        files++;
    }
    const Counters oneToOne = c;
    /* hand-made: root, two leaves.  Two leaves that name triangle 0 of two; then a triangle that no leaf names (three records) */
    unsigned long long handMade = 0;
    for (int which = 0; which < 2; which++) {
        Tree tree;
        const float box[3][6] = { { 0, 1, 0, 0, 1, 1 }, { 0, 0.5f, 0, 0, 1, 1 }, { 0.5f, 1, 0, 0, 1, 1 } };
        tree.w.resize(24);
        for (int i = 0; i < 3; i++)
            memcpy(&tree.w[8 * (size_t)i], box[i], 24);
        tree.w[6] = 3;
        tree.w[7] = NODE_CHILD | 1u;
        tree.w[8 + 6] = 2;
        tree.w[8 + 7] = 0;
        tree.w[16 + 6] = 3;
        tree.w[16 + 7] = which == 0 ? 0u : 1u;
        tree.tris.resize(which == 0 ? 2 : 3);
        for (size_t k = 0; k < tree.tris.size(); k++) {
            wpt_tri_geom& g = tree.tris[k];
            g.v0[0] = 0.1f + 0.5f * (float)(k & 1u); g.v0[1] = 0.1f; g.v0[2] = 0.2f;
            g.v1[0] = 0.4f + 0.5f * (float)(k & 1u); g.v1[1] = 0.1f; g.v1[2] = 0.5f;
            g.v2[0] = 0.2f + 0.5f * (float)(k & 1u); g.v2[1] = 0.9f; g.v2[2] = 0.8f;
        }
        Counters h;
        check(tree, false, false, 3000u + (uint32_t)which, h);
        printf("hand-made tree %d (%s): wrong verdicts %llu, wrong words %llu, walks %llu, walks that differ %llu\n", which,
                which == 0 ? "two leaves name one triangle" : "a triangle no leaf names", h.wrongVerdicts, h.wrongWords, h.walks, h.differ);
        handMade += h.wrongVerdicts == 0 && h.wrongWords == 0 && h.differ == 0 && h.walks > 0 ? 1 : 0;
    }
    const std::vector<uint32_t> none(4, 0u);
    const bool tooLarge = wptw::leafWords(none.data(), wptw::LEAF_NODE_MAX + 1, 0).verdict == wptw::TOO_LARGE
            && wptw::leafWords(none.data(), 0, wptw::LEAF_CORNER_MASK / 3 + 1).verdict == wptw::TOO_LARGE
            && wptw::leafWords(none.data(), 0, 0).verdict == wptw::ONE_TO_ONE;
    c = oneToOne;
    printf("trees %llu (%llu from files, %llu with a NaN bound), sets of link words %llu, leaves %llu\n", c.trees, files, nanTrees, c.sets, c.leaves);
    printf("empty nodes %llu, nodes whose link the fold changes %llu, nodes left out %llu\n", emptyNodes, foldedNodes, bypassedNodes);
    printf("walks %llu (%llu on the exact links throughout, %llu with the links taking turns), leaf tests of the model that reads the node %llu\n", c.walks, c.nanWalks, c.mixedWalks, c.leafTests);
    printf("wrong words: %llu\n", c.wrongWords);
    printf("wrong verdicts: %llu\n", c.wrongVerdicts);
    printf("hand-made trees judged not one to one: %llu of 2\n", handMade);
    printf("indices beyond the word refused: %s\n", tooLarge ? "yes" : "NO");
    const bool covered = nanTrees > 0 && emptyNodes > 0 && foldedNodes > 0 && bypassedNodes > 0 && c.nanWalks > 0 && c.mixedWalks > 0 && c.leafTests > 0 && c.leaves > 0;
    printf("cases covered: %s\n", covered ? "yes" : "NO");
    printf("walks that differ: %llu\n", c.differ);
    return c.differ == 0 && c.wrongWords == 0 && c.wrongVerdicts == 0 && handMade == 2 && tooLarge && covered ? 0 : 1;
}
