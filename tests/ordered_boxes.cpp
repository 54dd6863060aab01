// Harness of tests/test_ordered_boxes.py: the ordered box test of the 1024-lane kernels with the scene in LDS and the node copies
// it reads (wurblpt_amd/csrc/wpt_scene_layout.h, orderedBoxCopies -- the code wpt_scene_upload runs; wpt_device.h, boxTestOrdered
// and boxTest, restated on the host).  A ray whose slab distances are numbers walks with its negative axes mirrored (origin and
// reciprocal negated) and reads the copy of the node array whose bounds are mirrored the same way; its box test then sorts
// nothing.  Three parts:
//   1. verdicts: the ordered test on the mirrored ray and the mirrored record against boxTest<false> and boxTest<true> on the
//      originals, for random pairs (the count is argv[1], 10^7 by default) and for adversarial ones in all eight octants: the
//      origin on a bound, bounds +-0, lo == hi, infinite bounds, amax and amin equal to a slab distance, denormal reciprocals.
//      Rays with RAY_MAY_NAN do not take the ordered test and are only counted.  Beyond the verdict the two numbers that are
//      compared must be equal as numbers (the sign of a zero apart).
//   2. layout: copy 0 is the plain array with its padding node byte for byte, every other copy has the mirrored bounds and the
//      same links, and a tree with one inverted box or one NaN bound is refused.
//   3. walks: over the trees of tests/leaf_words.cpp's generator (300 random ones, the one that fills LDS) and the trees of the
//      files named behind the count (the Cornell box's), a model of the walk with the ordered step visits the nodes the present
//      step visits, in the same order with the same bounds, under every pair of link sets, also when looks take the NaN form
//      by the toss of a coin (a mixed group: mirrored lanes then take the sorting test on their own copy) and for rays with
//      RAY_MAY_NAN, which stay unmirrored on copy 0.  Trees without copies (a NaN bound) keep the present step and are counted.
#define main leaf_words_main /* the generator and the walk's leaf model are that program's own */
#include "leaf_words.cpp"
#undef main

#include "../wurblpt_amd/csrc/wpt_scene_layout.h"

namespace {

struct Box { float lo[3], hi[3]; };

// wpt_device.h, boxTest<CHECK> on (lo, hi, org, inv); *tmin, *tmax: the two numbers of the plain form
bool presentTest(const float* lo, const float* hi, const float* o, const float* inv, float amin, float amax, bool check, float* tminOut, float* tmaxOut)
{
    float t0[3], t1[3];
    for (int a = 0; a < 3; a++) {
        t0[a] = (lo[a] - o[a]) * inv[a];
        t1[a] = (hi[a] - o[a]) * inv[a];
    }
    const float tmin = fmaxf(fmaxf(fminf(t0[0], t1[0]), fminf(t0[1], t1[1])), fmaxf(fminf(t0[2], t1[2]), amin));
    const float tmax = fminf(fminf(fmaxf(t0[0], t1[0]), fmaxf(t0[1], t1[1])), fminf(fmaxf(t0[2], t1[2]), amax));
    bool hit = tmin <= tmax;
    if (check && (t0[0] != t0[0] || t1[0] != t1[0] || t0[1] != t0[1] || t1[1] != t1[1] || t0[2] != t0[2] || t1[2] != t1[2])) {
        float lo2 = amin, hi2 = amax; /* boxTestChains */
        for (int a = 0; a < 3; a++) {
            const float mn = t0[a] < t1[a] ? t0[a] : t1[a], mx = t0[a] > t1[a] ? t0[a] : t1[a];
            if (mn > lo2) lo2 = mn;
            if (mx < hi2) hi2 = mx;
        }
        hit = lo2 <= hi2;
    }
    if (tminOut) {
        *tminOut = tmin;
        *tmaxOut = tmax;
    }
    return hit;
}

// wpt_device.h, boxTestOrdered
bool orderedTest(const float* lo, const float* hi, const float* O, const float* I, float amin, float amax, float* tminOut, float* tmaxOut)
{
    float n[3], f[3];
    for (int a = 0; a < 3; a++) {
        n[a] = (lo[a] - O[a]) * I[a];
        f[a] = (hi[a] - O[a]) * I[a];
    }
    const float tmin = fmaxf(fmaxf(fmaxf(n[0], n[1]), n[2]), amin);
    const float tmax = fminf(fminf(fminf(f[0], f[1]), f[2]), amax);
    if (tminOut) {
        *tminOut = tmin;
        *tmaxOut = tmax;
    }
    return tmin <= tmax;
}

// the record of a device node (lo.x hi.x lo.y lo.z | hi.y hi.z skip word) as bounds
void recordBox(const wptl::Quad* q, float* lo, float* hi)
{
    lo[0] = q[0].x; hi[0] = q[0].y; lo[1] = q[0].z; lo[2] = q[0].w; hi[1] = q[1].x; hi[2] = q[1].y;
}

// beginRay of the ordered form: the octant, the mirrored origin and reciprocals
uint32_t mirror(const Ray& r, float* O, float* I)
{
    uint32_t k = 0;
    for (int a = 0; a < 3; a++) {
        const bool neg = !r.mayNan && std::signbit(r.inv[a]);
        k |= neg ? 1u << a : 0u;
        O[a] = neg ? -r.o[a] : r.o[a];
        I[a] = neg ? -r.inv[a] : r.inv[a];
    }
    return k;
}

struct Verdicts {
    unsigned long long pairs = 0, mayNan = 0, differ = 0, numbersDiffer = 0, hits = 0, octant[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
};

// a batch of (ray, box, amin, amax): the boxes become one node array, whose copies the layout function makes
void judge(std::vector<Ray>& rays, const std::vector<Box>& boxes, const std::vector<float>& amin, const std::vector<float>& amax, Verdicts& v)
{
    const uint32_t n = (uint32_t)boxes.size();
    std::vector<uint32_t> words(8 * (size_t)n, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const float rec[6] = { boxes[i].lo[0], boxes[i].hi[0], boxes[i].lo[1], boxes[i].lo[2], boxes[i].hi[1], boxes[i].hi[2] };
        memcpy(&words[8 * (size_t)i], rec, 24);
    }
    std::vector<wptl::Quad> copies;
    if (!wptl::orderedBoxCopies(words.data(), n, &copies)) {
        v.differ += n; /* every box here has lo <= hi */
        return;
    }
    const size_t stride = 2 * (size_t)n + 2;
    for (uint32_t i = 0; i < n; i++) {
        Ray& r = rays[i];
        finish(r);
        v.pairs++;
        if (r.mayNan) {
            v.mayNan++;
            continue;
        }
        float O[3], I[3], lo[3], hi[3], tmin[2], tmax[2];
        const uint32_t k = mirror(r, O, I);
        v.octant[k]++;
        recordBox(&copies[k * stride + 2 * (size_t)i], lo, hi);
        const bool ordered = orderedTest(lo, hi, O, I, amin[i], amax[i], &tmin[0], &tmax[0]);
        const bool plain = presentTest(boxes[i].lo, boxes[i].hi, r.o, r.inv, amin[i], amax[i], false, &tmin[1], &tmax[1]);
        const bool checked = presentTest(boxes[i].lo, boxes[i].hi, r.o, r.inv, amin[i], amax[i], true, nullptr, nullptr);
        /* a mixed group: the sorting test on the mirrored ray and record */
        const bool mixed = presentTest(lo, hi, O, I, amin[i], amax[i], true, nullptr, nullptr);
        v.hits += plain ? 1 : 0;
        if (ordered != plain || ordered != checked || mixed != plain)
            v.differ++;
        if (!(tmin[0] == tmin[1]) || !(tmax[0] == tmax[1]))
            v.numbersDiffer++;
    }
}

float special(Lcg& rng, int kind)
{
    switch (kind) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return INFINITY;
    case 3: return -INFINITY;
    case 4: return 1.0e-40f; /* denormal */
    case 5: return -1.0e-40f;
    default: return (float)(-2.0 + 4.0 * rng.unit());
    }
}

void randomPairs(unsigned long long count, Verdicts& v)
{
    Lcg rng = { 0x0bdeull };
    const uint32_t batch = 4096;
    std::vector<Ray> rays(batch);
    std::vector<Box> boxes(batch);
    std::vector<float> amin(batch), amax(batch);
    for (unsigned long long done = 0; done < count; done += batch) {
        for (uint32_t i = 0; i < batch; i++) {
            for (int a = 0; a < 3; a++) {
                const float p = (float)(-1.0 + 2.0 * rng.unit()), q = (float)(-1.0 + 2.0 * rng.unit());
                boxes[i].lo[a] = fminf(p, q);
                boxes[i].hi[a] = rng.unit() < 0.05 ? boxes[i].lo[a] : fmaxf(p, q);
                rays[i].o[a] = (float)(-2.0 + 4.0 * rng.unit());
                rays[i].d[a] = (float)(-1.0 + 2.0 * rng.unit());
                if (rng.unit() < 0.02) /* on a bound */
                    rays[i].o[a] = rng.unit() < 0.5 ? boxes[i].lo[a] : boxes[i].hi[a];
                if (rng.unit() < 0.01)
                    rays[i].d[a] *= 1.0e-6f;
            }
            amin[i] = 1.0e-4f;
            amax[i] = rng.unit() < 0.5 ? 3.0e38f : (float)(4.0 * rng.unit());
        }
        judge(rays, boxes, amin, amax, v);
    }
}

// every octant times every kind of special value per axis, for origins, bounds and bounds of the distance
void adversarialPairs(Verdicts& v)
{
    Lcg rng = { 0xad5eull };
    std::vector<Ray> rays;
    std::vector<Box> boxes;
    std::vector<float> amin, amax;
    for (int octant = 0; octant < 8; octant++)
        for (int kind = 0; kind < 12; kind++)
            for (int rep = 0; rep < 400; rep++) {
                Ray r;
                Box b;
                float mn = 1.0e-4f, mx = 3.0e38f;
                for (int a = 0; a < 3; a++) {
                    const float p = (float)(-1.0 + 2.0 * rng.unit()), q = (float)(-1.0 + 2.0 * rng.unit());
                    b.lo[a] = fminf(p, q);
                    b.hi[a] = fmaxf(p, q);
                    r.o[a] = (float)(-2.0 + 4.0 * rng.unit());
                    r.d[a] = (float)(0.05 + rng.unit()) * ((octant >> a) & 1 ? -1.0f : 1.0f);
                }
                const int a = (int)(rng.next() % 3u), c = (int)(rng.next() % 3u);
                switch (kind) {
                case 0: r.o[a] = b.lo[a]; break;                                   /* the origin on a bound */
                case 1: r.o[a] = b.hi[a]; r.o[c] = b.lo[c]; break;
                case 2: b.lo[a] = special(rng, rep % 2); b.hi[a] = special(rng, (rep / 2) % 2); r.o[a] = special(rng, (rep / 4) % 2 ? 6 : (rep / 8) % 2); break; /* bounds +-0 */
                case 3: b.hi[a] = b.lo[a]; if (rep % 2) r.o[a] = b.lo[a]; break;  /* lo == hi */
                case 4: b.lo[a] = -INFINITY; if (rep % 2) b.hi[c] = INFINITY; break; /* infinite bounds */
                case 5: for (int x = 0; x < 3; x++) { b.lo[x] = -INFINITY; b.hi[x] = INFINITY; } break;
                case 6: b.hi[a] = INFINITY; b.lo[a] = rep % 2 ? INFINITY : b.lo[a]; break;
                case 7: mx = ((rep % 2 ? b.lo[a] : b.hi[a]) - r.o[a]) * (1.0f / r.d[a]); break; /* amax a slab distance */
                case 8: mn = ((rep % 2 ? b.lo[a] : b.hi[a]) - r.o[a]) * (1.0f / r.d[a]); break; /* amin a slab distance */
                case 9: r.d[a] = ((octant >> a) & 1 ? -1.0f : 1.0f) * (2.0e38f + 1.0e38f * (float)rng.unit()); break; /* a denormal reciprocal */
                case 10: for (int x = 0; x < 3; x++) r.d[x] = ((octant >> x) & 1 ? -1.0f : 1.0f) * 3.0e38f; r.o[a] = b.lo[a]; break;
                default: r.d[a] = special(rng, rep % 6); r.o[c] = special(rng, 2 + rep % 3); break; /* rays that carry RAY_MAY_NAN */
                }
                if (!(b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2]))
                    continue;
                rays.push_back(r);
                boxes.push_back(b);
                amin.push_back(mn);
                amax.push_back(mx);
            }
    judge(rays, boxes, amin, amax, v);
}

struct Layout { unsigned long long trees = 0, copies = 0, wrong = 0, refusedInverted = 0, refusedNan = 0, notRefused = 0; };

bool sameBits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// part 2 for one tree; returns its copies (empty: the tree has none)
std::vector<wptl::Quad> layoutOf(const Tree& t, bool expectCopies, Layout& l)
{
    const uint32_t n = t.nodes();
    const size_t stride = 2 * (size_t)n + 2;
    std::vector<wptl::Quad> copies;
    const bool made = wptl::orderedBoxCopies(t.w.data(), n, &copies);
    l.trees++;
    if (made != expectCopies || (!made && !copies.empty()) || (made && copies.size() != wptl::ORDERED_COPIES * stride)) {
        l.wrong++;
        return std::vector<wptl::Quad>();
    }
    if (!made)
        return copies;
    std::vector<uint32_t> padded(t.w);
    padded.resize(4 * stride, 0u);
    if (memcmp(copies.data(), padded.data(), 16 * stride) != 0)
        l.wrong++;
    for (uint32_t k = 0; k < wptl::ORDERED_COPIES; k++) {
        l.copies++;
        for (uint32_t i = 0; i <= n; i++) {
            const wptl::Quad *p = &copies[2 * (size_t)i], *q = &copies[k * stride + 2 * (size_t)i];
            float plo[3], phi[3], lo[3], hi[3];
            recordBox(p, plo, phi);
            recordBox(q, lo, hi);
            bool ok = sameBits(p[1].z, q[1].z) && sameBits(p[1].w, q[1].w);
            for (int a = 0; a < 3; a++) {
                const bool neg = ((k >> a) & 1u) != 0 && i < n;
                ok = ok && sameBits(lo[a], neg ? -phi[a] : plo[a]) && sameBits(hi[a], neg ? -plo[a] : phi[a]);
            }
            l.wrong += ok ? 0 : 1;
        }
    }
    /* one inverted box, one NaN bound: no copies */
    if (n > 0) {
        Lcg rng = { 0x1a70ull + n };
        for (int which = 0; which < 2; which++) {
            Tree bad = t;
            const uint32_t i = rng.next() % n, a = rng.next() % 3u;
            const uint32_t at[3][2] = { { 0, 1 }, { 2, 4 }, { 3, 5 } }; /* lo, hi of axis a in the record */
            float lo, hi;
            memcpy(&lo, &bad.w[8 * (size_t)i + at[a][0]], 4);
            memcpy(&hi, &bad.w[8 * (size_t)i + at[a][1]], 4);
            if (which == 0) {
                lo = hi + 1.0f;
                if (!(lo > hi))
                    continue; /* (an infinite bound) */
                memcpy(&bad.w[8 * (size_t)i + at[a][0]], &lo, 4);
            } else {
                const float nan = NAN;
                memcpy(&bad.w[8 * (size_t)i + at[a][rng.next() % 2u]], &nan, 4);
            }
            std::vector<wptl::Quad> none;
            if (wptl::orderedBoxCopies(bad.w.data(), n, &none) || !none.empty())
                l.notRefused++;
            else
                (which == 0 ? l.refusedInverted : l.refusedNan)++;
        }
    }
    return copies;
}

struct Visit { uint32_t node, boundBits; };
struct Walks { unsigned long long trees = 0, treesWithoutCopies = 0, walks = 0, visits = 0, nanWalks = 0, mixedWalks = 0, mirroredWalks = 0, differ = 0; };

// A ray's walk as the kernels with the scene in LDS perform it (ldsStep and the leaf pass; tests/leaf_words.cpp, walk, FROM_NODE),
// with the nodes it visits.  copies == NULL: the present step on the plain record; else the ordered form.
std::vector<Visit> visitNodes(const Tree& t, const std::vector<wptl::Quad>* copies, const std::vector<uint32_t>& launch, const std::vector<uint32_t>& exact,
        const Ray& r, bool mixed)
{
    const uint32_t n = t.nodes();
    const size_t stride = 2 * (size_t)n + 2;
    std::vector<Visit> out;
    float amax = 3.0e38f, O[3], I[3];
    const uint32_t k = mirror(r, O, I);
    Lcg coin = { 0x51ull + r.id };
    uint32_t node = r.mayNan ? 0u : launch[2 * (size_t)n + 2];
    for (uint32_t looks = 0; node < n && looks < 100000; looks++) {
        bool nan = r.mayNan;
        if (!nan && mixed)
            nan = (coin.next() & 1u) != 0;
        const std::vector<uint32_t>& use = nan ? exact : launch;
        uint32_t bits;
        memcpy(&bits, &amax, 4);
        out.push_back({ node, bits });
        bool hit;
        if (copies) {
            float lo[3], hi[3];
            recordBox(&(*copies)[k * stride + 2 * (size_t)node], lo, hi);
            hit = nan ? presentTest(lo, hi, O, I, 1e-4f, amax, true, nullptr, nullptr) : orderedTest(lo, hi, O, I, 1e-4f, amax, nullptr, nullptr);
        } else {
            hit = boxTest(&t.w[8 * (size_t)node], r, 1e-4f, amax, nan);
        }
        const uint32_t skip = use[2 * (size_t)node], word = use[2 * (size_t)node + 1];
        if (!(hit && (int32_t)word < 0)) {
            node = hit ? word : skip;
            continue;
        }
        if (!r.mayNan && mixed)
            nan = (coin.next() & 1u) != 0;
        leafTest(~launch[2 * (size_t)node + 1], r.id, amax);
        node = nan ? exact[2 * (size_t)node] : launch[2 * (size_t)node];
    }
    return out;
}

void walkTree(const Tree& t, const std::vector<wptl::Quad>& copies, uint32_t seed, Walks& w)
{
    const uint32_t n = t.nodes(), m = (uint32_t)t.tris.size();
    w.trees++;
    if (copies.empty()) {
        w.treesWithoutCopies++;
        return;
    }
    const Plan p = plan(t.w.data(), n, t.tris.data(), m, MODE_MODEL);
    const std::vector<uint32_t>* sets[3] = { &p.plain, &p.folded, &p.bypass };
    std::vector<Ray> rays;
    std::vector<SampleRay> sample;
    sampleCounts(t.w.data(), n, t.tris.data(), m, &sample);
    for (size_t i = 0; i < sample.size() && rays.size() < 24; i += sample.size() / 24 + 1) {
        Ray r;
        memcpy(r.o, sample[i].o, 12);
        memcpy(r.d, sample[i].d, 12);
        rays.push_back(r);
    }
    float rootLo[3], rootHi[3];
    nodeBox(t.w.data(), 0, rootLo, rootHi);
    Lcg rng = { 0x0b0cull + seed };
    for (int q = 0; q < 24; q++) {
        Ray r;
        for (int a = 0; a < 3; a++) {
            r.o[a] = (float)(-1.0 + 3.0 * rng.unit());
            r.d[a] = rootLo[a] + (float)rng.unit() * (rootHi[a] - rootLo[a]) - r.o[a];
        }
        if (q % 4 == 3) { /* a zero component, often from a slab plane: RAY_MAY_NAN */
            const int a = (int)(rng.next() % 3u);
            r.d[a] = rng.unit() < 0.5 ? 0.0f : -0.0f;
            float lo[3], hi[3];
            nodeBox(t.w.data(), rng.next() % n, lo, hi);
            if (rng.unit() < 0.7)
                r.o[a] = rng.unit() < 0.5 ? lo[a] : hi[a];
            if (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f)
                r.d[rng.next() % 3u] = 1.0f;
        }
        rays.push_back(r);
    }
    for (size_t q = 0; q < rays.size(); q++) {
        Ray& r = rays[q];
        r.id = seed * 64u + (uint32_t)q;
        finish(r);
        const int pairs[3][2] = { { 0, 0 }, { 1, 1 }, { 1, 2 } };
        for (int k = 0; k < 3; k++)
            for (int mixed = 0; mixed < 2; mixed++) {
                const std::vector<Visit> present = visitNodes(t, nullptr, *sets[pairs[k][1]], *sets[pairs[k][0]], r, mixed != 0);
                const std::vector<Visit> ordered = visitNodes(t, &copies, *sets[pairs[k][1]], *sets[pairs[k][0]], r, mixed != 0);
                w.walks++;
                w.visits += present.size();
                w.nanWalks += r.mayNan ? 1 : 0;
                w.mixedWalks += mixed;
                w.mirroredWalks += !r.mayNan && (std::signbit(r.inv[0]) || std::signbit(r.inv[1]) || std::signbit(r.inv[2])) ? 1 : 0;
                bool same = present.size() == ordered.size();
                for (size_t i = 0; same && i < present.size(); i++)
                    same = present[i].node == ordered[i].node && present[i].boundBits == ordered[i].boundBits;
                w.differ += same ? 0 : 1;
            }
    }
}

} // namespace

int main(int argc, char** argv)
{
    const unsigned long long count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    Verdicts random, adversarial;
    randomPairs(count, random);
    adversarialPairs(adversarial);
    printf("random pairs %llu (%llu with RAY_MAY_NAN, %llu hits), octants", random.pairs, random.mayNan, random.hits);
    for (int k = 0; k < 8; k++)
        printf(" %llu", random.octant[k]);
    printf("\nadversarial pairs %llu (%llu with RAY_MAY_NAN, %llu hits), octants", adversarial.pairs, adversarial.mayNan, adversarial.hits);
    for (int k = 0; k < 8; k++)
        printf(" %llu", adversarial.octant[k]);
    printf("\ndiffering verdicts: %llu\n", random.differ + adversarial.differ);
    printf("differing distances: %llu\n", random.numbersDiffer + adversarial.numbersDiffer);
    bool octants = true;
    for (int k = 0; k < 8; k++)
        octants = octants && random.octant[k] > 0 && adversarial.octant[k] > 0;

    Layout l;
    Walks w;
    unsigned long long files = 0;
    for (int i = 0; i < 300; i++) {
        Tree tree;
        Lcg rng = { 0x1ea5ull + 104729ull * (uint64_t)i };
        grow(tree, rng, 1 + (int)(rng.next() % 200u), nullptr, nullptr);
        bool nanTree = false;
        if (i % 10 == 9) {
            uint32_t bits;
            const float nan = NAN;
            memcpy(&bits, &nan, 4);
            tree.w[8 * (size_t)(rng.next() % tree.nodes()) + rng.next() % 6u] = bits;
            nanTree = true;
        }
        walkTree(tree, layoutOf(tree, !nanTree, l), (uint32_t)i, w);
    }
    {
        Tree big;
        uint32_t leaves = 0;
        const float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
        halve(big, leaves, 289, lo, hi, 0);
        walkTree(big, layoutOf(big, true, l), 1000u, w);
    }
    for (int a = 2; a < argc; a++) {
        Tree tree;
        if (!load(argv[a], tree)) {
            printf("cannot read %s\n", argv[a]);
            return 2;
        }
        const std::vector<wptl::Quad> copies = layoutOf(tree, true, l);
        printf("tree of %s: %u nodes, %zu triangles, %s\n", argv[a], tree.nodes(), tree.tris.size(), copies.empty() ? "NO ordered copies" : "ordered copies");
        walkTree(tree, copies, 2000u + (uint32_t)a, w);
        files++;
    }
    printf("layout: trees %llu (%llu from files), copies checked %llu, wrong %llu; refused with an inverted box %llu, with a NaN bound %llu, not refused %llu\n",
            l.trees, files, l.copies, l.wrong, l.refusedInverted, l.refusedNan, l.notRefused);
    printf("walks: trees %llu (%llu without copies), walks %llu (%llu with RAY_MAY_NAN, %llu mixed, %llu mirrored), node visits %llu\n",
            w.trees, w.treesWithoutCopies, w.walks, w.nanWalks, w.mixedWalks, w.mirroredWalks, w.visits);
    printf("walks that differ: %llu\n", w.differ);
    const bool covered = octants && random.pairs >= count && adversarial.mayNan > 0 && random.hits > 0 && l.refusedInverted > 0 && l.refusedNan > 0
            && w.nanWalks > 0 && w.mixedWalks > 0 && w.mirroredWalks > 0 && w.visits > 0 && w.treesWithoutCopies > 0;
    printf("cases covered: %s\n", covered ? "yes" : "NO");
    return random.differ + adversarial.differ == 0 && random.numbersDiffer + adversarial.numbersDiffer == 0 && l.wrong == 0 && l.notRefused == 0
            && w.differ == 0 && covered ? 0 : 1;
}
