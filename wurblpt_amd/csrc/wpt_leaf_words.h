/*
 * wpt_leaf_words.h -- what the leaf pass of the kernels with rotated corner copies reads instead of the leaf's node (host only).
 *
 * A leaf's node gives its test three things: the triangle, the node the walk goes on at (its skip link under the launch's links)
 * and, for a group with RAY_MAY_NAN rays, the exact skip link.  Read from the node they cost the leaf pass an LDS round trip
 * before the one that fetches the corners.  Where every triangle is named by exactly one leaf, the three are a function of the
 * triangle: they ride in the fourth words of the triangle's three corner records in LDS, which the test fetches anyway, and the
 * node step keeps the leaf's word -- which says where those records lie -- in the place of the leaf's index.
 *
 * The leaf word of these kernels (the sign bit still tells a leaf from an inner node, whose word is an index < 2^30):
 *     LEAF_BIT | leaf's node index << LEAF_NODE_SHIFT | 3 * triangle      (the quadword offset of the triangle's first corner)
 * The node index is there for the trees that are not one-to-one (the C ABI admits two leaves with one triangle): their leaf pass
 * reads the skip links from the node as before, and only the triangle's index from the record.
 *
 * One set of link words in (wpt_bypass.h, linkWords: plain, folded or bypass), one set out: the same pairs with the leaf words
 * recoded, and behind them per triangle the skip link of its leaf under that set.  A pure function of the tree.
 */
#ifndef WPT_LEAF_WORDS_H
#define WPT_LEAF_WORDS_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace wptw {

constexpr uint32_t LEAF_BIT = 0x80000000u;
constexpr uint32_t LEAF_NODE_SHIFT = 16;
constexpr uint32_t LEAF_NODE_MAX = 0x7fffu;    /* node indices the word has room for */
constexpr uint32_t LEAF_CORNER_MASK = 0xffffu; /* 3 * triangle */

enum Verdict {
    ONE_TO_ONE = 0,     /* every triangle is named by exactly one leaf and every leaf names a triangle */
    NOT_ONE_TO_ONE = 1, /* the leaf pass must take the skip links from the leaf's node */
    TOO_LARGE = 2       /* the tree's indices do not fit the leaf word: no words made (no tree that fits LDS is that large) */
};

inline uint32_t leafWord(uint32_t node, uint32_t triangle) { return LEAF_BIT | (node << LEAF_NODE_SHIFT) | (3u * triangle); }
inline uint32_t leafWordNode(uint32_t word) { return (word >> LEAF_NODE_SHIFT) & LEAF_NODE_MAX; }
inline uint32_t leafWordCorner(uint32_t word) { return word & LEAF_CORNER_MASK; }

/* words of a set made by leafWords: the pairs of linkWords, then one word per triangle, padded to whole pairs */
inline size_t leafWordsSize(uint32_t nodeCount, uint32_t triCount) { return 2 * size_t(nodeCount) + 4 + ((size_t(triCount) + 1) & ~size_t(1)); }
/* where the per-triangle words start */
inline size_t leafWordsTriangles(uint32_t nodeCount) { return 2 * size_t(nodeCount) + 4; }

struct LeafWords {
    std::vector<uint32_t> words; /* leafWordsSize(); a triangle no leaf names has nodeCount for its skip link */
    Verdict verdict;
};

/* links: 2 * nodeCount + 4 words (skip link, word 7 of the LDS copy: an index, or a leaf's triangle complemented) */
inline LeafWords leafWords(const uint32_t* links, uint32_t nodeCount, uint32_t triCount)
{
    LeafWords r;
    r.verdict = ONE_TO_ONE;
    if (nodeCount > LEAF_NODE_MAX || 3 * uint64_t(triCount) > LEAF_CORNER_MASK) {
        r.verdict = TOO_LARGE;
        return r;
    }
    const size_t tris = leafWordsTriangles(nodeCount);
    r.words.assign(links, links + tris);
    r.words.resize(leafWordsSize(nodeCount, triCount), nodeCount);
    std::vector<uint32_t> named(triCount, 0u);
    for (uint32_t i = 0; i < nodeCount; i++) {
        const uint32_t word = links[2 * size_t(i) + 1];
        if (!(word & LEAF_BIT))
            continue;
        const uint32_t triangle = ~word;
        if (triangle >= triCount) {
            /* a leaf that names no triangle: the word of triangle 0's place keeps the walk inside the records, the verdict
             * keeps such a tree away from the kernels (the upload refuses it before) */
            r.words[2 * size_t(i) + 1] = leafWord(i, 0u);
            r.verdict = NOT_ONE_TO_ONE;
            continue;
        }
        r.words[2 * size_t(i) + 1] = leafWord(i, triangle);
        r.words[tris + triangle] = links[2 * size_t(i)];
        named[triangle] += 1;
    }
    for (uint32_t t = 0; t < triCount; t++)
        if (named[t] != 1)
            r.verdict = NOT_ONE_TO_ONE;
    return r;
}

} // namespace wptw

#endif
