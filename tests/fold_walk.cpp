// Harness of tests/test_fold_walk.py: wptf::foldLdsWord (wurblpt_amd/csrc/wpt_fold.h), the rule by which the kernels with the
// scene in LDS fold first children that repeat their parent's box out of their copy of the tree -- the code the kernels'
// prologue and wpt_scene_upload run.  Random depth-first trees of up to 200 nodes in which a chosen share of first children copy
// their parent's box (among them chains of three, chains from the root, leaf first children, empty nodes, second children with
// the parent's box and copies that differ in one bit) are walked with the stackless rule, unfolded over the device words and,
// with the fold and without it, over the LDS words as ldsStep and the leaf test of wpt_pathtrace.inc.h do.  The box predicate is a hash of (box bits, ray,
// epoch), where the epoch advances at every leaf test: it stands for any test that depends on the bound.  Per walk: the leaves
// tested are the same sequence, and the unfolded walk's visits minus the folded walk's are the unfolded walk's visits to folded
// children (counted from the transitions, without the rule's code).  No tolerance.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_fold.h"

using namespace wptf;

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
};

enum { INNER, LEAF, EMPTY };
struct Node { uint32_t box[6]; int kind; uint32_t second, prim; };

struct Gen {
    Rng rng;
    double share;
    std::vector<Node> nodes;
    uint32_t prims = 0;
    // a subtree of at most `budget` nodes; box: the parent's box if this is a child; chain: first children still to copy it
    uint32_t make(int budget, const uint32_t* parent, bool first, int chain)
    {
        const uint32_t i = (uint32_t)nodes.size();
        nodes.push_back(Node());
        Node nd;
        for (int k = 0; k < 6; k++)
            nd.box[k] = rng.next() ^ (rng.next() << 1);
        const double u = rng.unit();
        if (parent && ((first && (chain > 0 || u < share)) || (!first && u < 0.15))) {
            memcpy(nd.box, parent, sizeof(nd.box)); /* a second child's copy must never fold */
        } else if (parent && first && u < share + 0.1) {
            memcpy(nd.box, parent, sizeof(nd.box));
            nd.box[rng.next() % 6] ^= 1u << (rng.next() % 32); /* one bit off */
        }
        const bool inner = budget >= 3 && (chain > 1 || rng.unit() < 0.75);
        nd.second = nd.prim = 0;
        if (inner) {
            nd.kind = INNER;
            const int b1 = 1 + (int)(rng.next() % (uint32_t)(budget - 2));
            nodes[i] = nd;
            make(b1, nd.box, true, chain > 0 ? chain - 1 : 0);
            nd.second = make(budget - 1 - b1, nd.box, false, 0);
        } else if (rng.unit() < 0.1) {
            nd.kind = EMPTY;
        } else {
            nd.kind = LEAF;
            nd.prim = prims++;
        }
        nodes[i] = nd;
        return i;
    }
};

static bool pred(const uint32_t* box, uint32_t ray, uint32_t epoch)
{
    uint64_t h = 1469598103934665603ull;
    for (int k = 0; k < 6; k++)
        h = (h ^ box[k]) * 1099511628211ull;
    h = (h ^ ray) * 1099511628211ull;
    h = (h ^ epoch) * 1099511628211ull;
    h ^= h >> 29;
    return (h * 0x9e3779b97f4a7c15ull >> 40) % 100 < 72;
}

int main()
{
    unsigned long long trees = 0, walks = 0, bad = 0, visitsPlain = 0, saved = 0, leafTests = 0;
    unsigned long long foldedLinks = 0, leafFirstChildren = 0, rootChains = 0, chains3 = 0;
    const double shares[5] = { 0.0, 0.2, 0.5, 0.8, 1.0 };
    for (int t = 0; t < 3000; t++) {
        Gen g;
        g.rng.s = 0x1234567ull + 7919ull * (uint64_t)t;
        g.share = shares[t % 5];
        const int budget = 1 + (int)(g.rng.next() % 200u);
        g.make(budget, nullptr, false, (t % 7 == 0) ? 3 : 0); /* every seventh tree: a chain of three from the root */
        const uint32_t n = (uint32_t)g.nodes.size();
        if (n > 200) {
            printf("tree %d has %u nodes\n", t, n);
            return 2;
        }
        /* the device words, as wpt_scene_upload makes them */
        std::vector<uint32_t> end(n), w(8 * (size_t)n);
        for (uint32_t i = n; i-- > 0;)
            end[i] = g.nodes[i].kind == INNER ? end[g.nodes[i].second] : i + 1;
        for (uint32_t i = 0; i < n; i++) {
            memcpy(&w[8 * (size_t)i], g.nodes[i].box, 24);
            w[8 * (size_t)i + 6] = end[i];
            w[8 * (size_t)i + 7] = g.nodes[i].kind == INNER ? (FOLD_NODE_CHILD | (i + 1)) : g.nodes[i].kind == LEAF ? g.nodes[i].prim : (FOLD_NODE_CHILD | end[i]);
        }
        trees++;
        for (uint32_t i = 0; i < n; i++)
            if (g.nodes[i].kind == INNER && g.nodes[i + 1].kind == LEAF && memcmp(g.nodes[i].box, g.nodes[i + 1].box, 24) == 0)
                leafFirstChildren++; /* a leaf first child with its parent's box: not folded */
        for (int form = 0; form < 2; form++) { /* 0: WPT_WALK_NO_FOLD, 1: the fold */
            const bool fold = form != 0;
            /* the LDS copy: word 7 by the rule, skip links clamped, the null node behind the tree */
            std::vector<uint32_t> ldsWord(n + 1), ldsSkip(n + 1);
            for (uint32_t i = 0; i < n; i++) {
                uint32_t links;
                ldsWord[i] = foldLdsWord(w.data(), n, i, fold, &links);
                ldsSkip[i] = end[i] < n ? end[i] : n;
                if (fold) {
                    foldedLinks += links;
                    if (i == 0 && links > 0)
                        rootChains++;
                    if (links >= 3)
                        chains3++;
                } else if (links != 0) {
                    bad++;
                }
            }
            ldsWord[n] = ldsSkip[n] = n;
            for (uint32_t ray = 0; ray < 24; ray++) {
                const uint32_t id = (uint32_t)t * 64u + ray;
                /* unfolded: binaryStep over the device words */
                std::vector<uint32_t> seqA, seqB;
                unsigned long long visitsA = 0, visitsB = 0, toFolded = 0;
                uint32_t epoch = 0, node = 0;
                while (node < n) {
                    visitsA++;
                    const uint32_t* nd = &w[8 * (size_t)node];
                    const bool hit = pred(nd, id, epoch);
                    if (hit && nd[7] >= FOLD_NODE_CHILD) {
                        const uint32_t c = nd[7] & FOLD_INDEX_MASK;
                        /* a step from a node whose box the ray passes to a child with that box: the visit a fold saves */
                        if (fold && c < n && memcmp(nd, &w[8 * (size_t)c], 24) == 0 && w[8 * (size_t)c + 7] >= FOLD_NODE_CHILD)
                            toFolded++;
                        node = c;
                    } else {
                        if (hit) {
                            seqA.push_back(nd[7]);
                            epoch++;
                        }
                        node = nd[6];
                    }
                }
                /* folded: ldsStep and the leaf test's decoding */
                epoch = 0;
                node = 0;
                while (node < n) {
                    visitsB++;
                    const bool hit = pred(&w[8 * (size_t)node], id, epoch);
                    const uint32_t word = ldsWord[node];
                    if (hit && (int32_t)word < 0) {
                        seqB.push_back(~word);
                        epoch++;
                        node = ldsSkip[node];
                    } else {
                        node = hit ? word : ldsSkip[node];
                    }
                    if (visitsB > 100000)
                        break;
                }
                walks++;
                if (seqA != seqB || visitsA - visitsB != toFolded) {
                    if (bad < 10)
                        printf("tree %d form %d ray %u: %zu / %zu leaves, visits %llu / %llu, to folded children %llu\n", t, form, ray, seqA.size(), seqB.size(), visitsA, visitsB, toFolded);
                    bad++;
                }
                if (form == 0) {
                    visitsPlain += visitsA;
                    leafTests += seqA.size();
                } else {
                    saved += toFolded;
                }
            }
        }
    }
    printf("trees %llu, walks %llu, node visits %llu, leaf tests %llu\n", trees, walks, visitsPlain, leafTests);
    printf("folded links: %llu; chains from the root %llu, chains of three and more %llu; leaf first children with the parent's box %llu\n", foldedLinks, rootChains, chains3, leafFirstChildren);
    printf("visits saved: %llu\n", saved);
    const bool covered = foldedLinks > 0 && leafFirstChildren > 0 && rootChains > 0 && chains3 > 0 && saved > 0;
    printf("cases covered: %s\n", covered ? "yes" : "NO");
    printf("walks that differ: %llu\n", bad);
    return bad == 0 && covered ? 0 : 1;
}
