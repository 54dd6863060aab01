/*
 * wpt_fold.h -- word 7 of a node's copy in LDS (wpt_pathtrace.inc.h, the kernels with the scene in LDS), for host and device.
 *
 * The stackless walk goes from an inner node N whose box the ray passes to N's first child C and tests C's box next: no leaf
 * test runs in between and the bound does not change.  The box test is a pure function of (box, origin, reciprocals, amin,
 * amax), in its plain and in its NaN form alike, so where C's six bounds are N's bit for bit, C's test repeats N's on the same
 * inputs and gives the same answer.  The LDS copy takes that step without computing it: where C is inner (or empty), N's word
 * becomes C's child link -- along the whole chain of such children, which may start at the root.  N's skip link and C's own
 * record stay as they are; the node step is the same instructions.
 * A second child with its parent's box is never folded: the bound may have changed before its turn.  A first child that is a
 * leaf is not folded either (its parent would have to carry the leaf's triangle and skip link: measured, no gain beyond the
 * spread on the Cornell frame, profiles/fold_first_children_cornell.txt).
 * The same walk with fewer steps: the leaves tested, their order and every bound are the unfolded walk's.
 */
#ifndef WPT_FOLD_H
#define WPT_FOLD_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WPT_FOLD_HD __host__ __device__ __forceinline__
#else
#define WPT_FOLD_HD inline
#endif

namespace wptf {

/* the device node as eight words: 0 .. 5 the box, 6 the skip link, 7 a triangle index, or FOLD_NODE_CHILD | first child */
constexpr uint32_t FOLD_NODE_CHILD = 0xc0000000u;
constexpr uint32_t FOLD_INDEX_MASK = 0x3fffffffu;

WPT_FOLD_HD bool foldSameBox(const uint32_t* a, const uint32_t* b)
{
    return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3]) | (a[4] ^ b[4]) | (a[5] ^ b[5])) == 0u;
}

/* Word 7 of node i's copy in LDS.  An inner node: the index of the node a ray that passes its box goes to (links that leave
 * the tree: nodeCount, the null node); a leaf: its word complemented (>= 2^31; every index is below).  fold = false keeps an
 * inner node's own first child.  *links: the first children taken out of the walk behind this node, 0 if the word is the plain one. */
WPT_FOLD_HD uint32_t foldLdsWord(const uint32_t* nodes, uint32_t nodeCount, uint32_t i, bool fold, uint32_t* links)
{
    const uint32_t* n = nodes + 8 * (size_t)i;
    uint32_t word = n[7];
    *links = 0u;
    if (word < FOLD_NODE_CHILD)
        return ~word;
    if (fold) {
        /* (the bounds end a chain that a malformed tree closes to a ring) */
        for (uint32_t k = 0; k < nodeCount && k < 0xffffu; k++) {
            const uint32_t child = word & FOLD_INDEX_MASK;
            if (child >= nodeCount)
                break;
            const uint32_t* c = nodes + 8 * (size_t)child;
            if (!foldSameBox(n, c))
                break;
            if (c[7] >= FOLD_NODE_CHILD) {
                word = c[7];
                *links += 1u;
            } else {
                break;
            }
        }
    }
    const uint32_t child = word & FOLD_INDEX_MASK;
    return child < nodeCount ? child : nodeCount;
}

} // namespace wptf

#endif
