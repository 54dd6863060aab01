/*
 * wpt_scene_layout.h -- how a scene description becomes the arrays the kernels read (host only; wpt_capi_scene.hip).
 *
 * Every piece of arithmetic that decides what lies where on the device, each as a function of the description and of the two
 * option words that bear on it (the nodes in front of wpt_set_top_nodes, the WPT_WALK_* flags): validation, the triangles'
 * storage order, the stackless node form and its storage order, the wide form, the permuted triangle records and hot spots, the
 * decoded texel pool's offsets, the measured BRDFs' pool with its interleaved tables, and the environment's sampling tables.
 * No HIP call, nothing global, no header of the kernels, so that it is tested without a device and compiles on its own under the
 * host sanitizers (tests/scene_layout_check.cpp).  wpt_scene_upload calls these one array at a time -- lay out, copy, release --
 * so the host never holds more than one laid-out array of a large scene; wpt_fold_plan packs its nodes with deviceNodes too.
 * DESIGN.md section 3, "How a description becomes these arrays", names what each function makes.
 *
 * Every layout function expects a description that validate() accepted.
 */
#ifndef WPT_SCENE_LAYOUT_H
#define WPT_SCENE_LAYOUT_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/wurblpt_hip.h"
#include "wpt_fold.h"
#include "wpt_lds_places.h"
#include "wpt_rgl.h"

namespace wptl {

/* the kernels' node words and limits (wpt_device.h, wpt_pathtrace.inc.h), restated for a file that includes none of their
 * headers; wpt_capi.hip asserts that they agree */
constexpr uint32_t NODE_CHILD = 0xc0000000u, NODE_INDEX_MASK = 0x3fffffffu, PRIM_SPHERE = 0x80000000u;
constexpr uint32_t WIDE_STACK = 96, WIDE_NONE = 0xffffffffu;
constexpr uint32_t LDS_SCENE_MAX_BYTES = 20 * 1024;
static_assert(NODE_CHILD == wptf::FOLD_NODE_CHILD && NODE_INDEX_MASK == wptf::FOLD_INDEX_MASK, "wpt_fold.h reads the words deviceNodes writes");

/* a quadword as the device fetches it (upload hands them over as float4) */
struct Quad {
    float x, y, z, w;
};
static_assert(sizeof(Quad) == 16, "a quadword is 16 bytes");

inline Quad quad(float x, float y, float z, float w)
{
    const Quad q = { x, y, z, w };
    return q;
}

struct Status {
    wpt_status code;
    const char* message; /* a literal; NULL with WPT_OK */
};

inline Status refuse(wpt_status code, const char* message)
{
    const Status s = { code, message };
    return s;
}

inline Status validate(const wpt_scene_desc* d)
{
    if (!d)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "scene description is NULL");
    if (d->abi_version != WPT_ABI_VERSION)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "scene description has a different ABI version");
    if (d->node_count == 0 || !d->nodes)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "scene has no BVH nodes (run Scene::updateBVH)");
    /* an array with a count is an array: NULL is an error of the caller's, not a fault of this process */
    if (d->tri_count > 0 && !d->tri_geom)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "triangle geometry array (tri_geom) is NULL");
    if (d->tri_count > 0 && !d->tri_attr)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "triangle attribute array (tri_attr) is NULL");
    if (d->instance_count > 0 && !d->instances)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "instance array (instances) is NULL");
    if (d->material_count > 0 && !d->materials)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "material array (materials) is NULL");
    if (d->texture_count > 0 && !d->textures)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "texture array (textures) is NULL");
    if (d->hotspot_count > 0 && !d->hotspots)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "hot spot array (hotspots) is NULL");
    if (d->texel_bytes > 0 && !d->texels)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "texel pool (texels) is NULL");
    /* every index the kernel will follow must stay inside its array: a bad index would be an
     * out-of-bounds access on the GPU */
    for (uint32_t i = 0; i < d->node_count; i++) {
        const wpt_bvh_node& n = d->nodes[i];
        if (n.kind == WPT_NODE_INNER) {
            if (n.link >= d->node_count || n.link <= i || i + 1 >= d->node_count)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH inner node links outside the node array");
        } else if (n.kind == WPT_NODE_TRIANGLE) {
            if (n.link >= d->tri_count || n.link >= PRIM_SPHERE)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH leaf references a triangle outside the array");
        } else if (n.kind == WPT_NODE_SPHERE) {
            if (n.link >= d->sphere_count || n.link >= (NODE_CHILD & ~PRIM_SPHERE))
                return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH leaf references a sphere outside the array");
        } else if (n.kind != WPT_NODE_EMPTY) {
            return refuse(WPT_ERR_UNSUPPORTED, "BVH node kind is not known to the kernel");
        }
    }
    {
        /* ... and the links must describe ONE depth-first tree over all nodes: the first child of an inner node is the
         * next node, its second child (link) starts where the first child's subtree ends.  Links that are merely in
         * range could share children (the device form would grow without bound) or leave nodes unreachable (the walk
         * would run into records nobody wrote).  One reverse pass: end[i] = first node behind the subtree of node i. */
        std::vector<uint32_t> end(d->node_count);
        for (uint32_t i = d->node_count; i-- > 0;) {
            const wpt_bvh_node& n = d->nodes[i];
            if (n.kind == WPT_NODE_INNER) {
                if (n.link != end[i + 1])
                    return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH nodes are not one depth-first tree (second child does not follow the first child's subtree)");
                end[i] = end[n.link];
            } else {
                end[i] = i + 1;
            }
        }
        if (end[0] != d->node_count)
            return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH nodes are not one depth-first tree (nodes behind the root's subtree)");
    }
    for (uint32_t i = 0; i < d->tri_count; i++) {
        if (d->tri_geom[i].instance >= d->instance_count || d->tri_geom[i].material >= d->material_count)
            return refuse(WPT_ERR_INVALID_ARGUMENT, "triangle references an instance or material outside the arrays");
    }
    for (uint32_t i = 0; i < d->material_count; i++) {
        const wpt_material& m = d->materials[i];
        if (m.type > WPT_MAT_LIGHT_SPOT)
            return refuse(WPT_ERR_UNSUPPORTED, "material type is not known to the kernel");
        if ((m.flags & WPT_MATF_TOF_LIGHT) && m.type != WPT_MAT_LIGHT_SPOT)
            return refuse(WPT_ERR_INVALID_ARGUMENT, "only a spot light can be a time-of-flight light (WPT_MATF_TOF_LIGHT)");
        if (m.type == WPT_MAT_RGL) {
            if (m.tex[0] < 0 || uint32_t(m.tex[0]) >= d->rgl_count)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "material references a measured BRDF outside the array");
            if (m.normal_tex >= int32_t(d->texture_count))
                return refuse(WPT_ERR_INVALID_ARGUMENT, "material references a normal map outside the array");
            continue;
        }
        if (m.type == WPT_MAT_TWOSIDED) {
            if (m.tex[0] < 0 || m.tex[1] < 0 || uint32_t(m.tex[0]) >= d->material_count || uint32_t(m.tex[1]) >= d->material_count)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "two-sided material references a material outside the array");
        } else {
            for (int k = 0; k < 5; k++)
                if (m.tex[k] >= int32_t(d->texture_count))
                    return refuse(WPT_ERR_INVALID_ARGUMENT, "material references a texture outside the array");
        }
        if (m.normal_tex >= int32_t(d->texture_count))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "material references a normal map outside the array");
    }
    for (uint32_t i = 0; i < d->texture_count; i++) {
        const wpt_texture& t = d->textures[i];
        if (t.type > WPT_TEX_TRANSFORMER)
            return refuse(WPT_ERR_UNSUPPORTED, "texture type is not known to the kernel");
        if (t.type == WPT_TEX_TRANSFORMER && (t.child < 0 || uint32_t(t.child) >= d->texture_count || uint32_t(t.child) >= i))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "texture transformer references a texture outside the array");
        if (t.type == WPT_TEX_IMAGE) {
            size_t cs = t.texel_type == WPT_TEXEL_U8 ? 1 : t.texel_type == WPT_TEXEL_U16 ? 2 : 4;
            if (t.width == 0 || t.height == 0 || t.comps < 1 || t.comps > 4 || t.texel_type > WPT_TEXEL_F32
                    || t.texel_offset + size_t(t.width) * t.height * t.comps * cs > d->texel_bytes)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "image texture lies outside the texel pool");
        }
    }
    if (d->rgl_count > 0 && (!d->rgl_brdfs || !d->rgl_data))
        return refuse(WPT_ERR_INVALID_ARGUMENT, "measured BRDF arrays are NULL");
    for (uint32_t i = 0; i < d->rgl_count; i++) {
        /* every table of the model must lie inside the pool (the kernel indexes it with data-dependent offsets) */
        const wpt_rgl_brdf& b = d->rgl_brdfs[i];
        const wpt_rgl_warp* warps[5] = { &b.ndf, &b.sigma, &b.vndf, &b.luminance, &b.rgb };
        const uint32_t wantDims[5] = { 0, 0, 2, 2, 3 };
        for (int k = 0; k < 5; k++) {
            const wpt_rgl_warp& w = *warps[k];
            if (w.dims != wantDims[k] || w.size_x < 2 || w.size_y < 2)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "measured BRDF table has an unexpected shape");
            uint64_t slices = 1;
            for (uint32_t dim = 0; dim < w.dims; dim++) {
                if (w.param_size[dim] < 1 || uint64_t(w.param_values[dim]) + w.param_size[dim] > d->rgl_data_count)
                    return refuse(WPT_ERR_INVALID_ARGUMENT, "measured BRDF parameter grid lies outside the pool");
                slices *= w.param_size[dim];
            }
            const uint64_t n = uint64_t(w.size_x) * w.size_y;
            const bool cdf = k == 2 || k == 3;
            if (uint64_t(w.data) + slices * n > d->rgl_data_count
                    || (cdf && (w.marginal_cdf == WPT_RGL_NONE || w.conditional_cdf == WPT_RGL_NONE
                            || uint64_t(w.marginal_cdf) + slices * w.size_y > d->rgl_data_count
                            || uint64_t(w.conditional_cdf) + slices * n > d->rgl_data_count)))
                return refuse(WPT_ERR_INVALID_ARGUMENT, "measured BRDF table lies outside the pool");
        }
    }
    if (d->sphere_count > 0 && !d->spheres)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "sphere array is NULL");
    for (uint32_t i = 0; i < d->sphere_count; i++) {
        if (d->spheres[i].material >= d->material_count)
            return refuse(WPT_ERR_INVALID_ARGUMENT, "sphere references a material outside the array");
        if (d->spheres[i].animation >= int32_t(d->animation_count))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "sphere refers to an animation outside the array");
    }
    for (uint32_t i = 0; i < d->hotspot_count; i++) {
        const wpt_hotspot& h = d->hotspots[i];
        if (h.kind > WPT_HOTSPOT_SPHERE)
            return refuse(WPT_ERR_UNSUPPORTED, "hot spot kind is not known to the kernel");
        if (h.prim >= (h.kind == WPT_HOTSPOT_SPHERE ? d->sphere_count : d->tri_count))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "hot spot references a primitive outside the array");
    }
    if (d->animation_count > 0 && (!d->animations || (d->keyframe_count > 0 && !d->keyframes)))
        return refuse(WPT_ERR_INVALID_ARGUMENT, "animation arrays are NULL");
    for (uint32_t i = 0; i < d->animation_count; i++) {
        const wpt_animation& a = d->animations[i];
        if (uint64_t(a.first_keyframe) + a.keyframe_count > d->keyframe_count)
            return refuse(WPT_ERR_INVALID_ARGUMENT, "animation refers to key frames outside the array");
        for (uint32_t k = 1; k < a.keyframe_count; k++)
            if (!(d->keyframes[a.first_keyframe + k - 1].t < d->keyframes[a.first_keyframe + k].t))
                return refuse(WPT_ERR_INVALID_ARGUMENT, "key frames must be sorted by ascending time");
    }
    for (uint32_t i = 0; i < d->instance_count; i++) {
        const wpt_instance& inst = d->instances[i];
        if (inst.animation >= int32_t(d->animation_count) || ((inst.flags & WPT_TRI_ANIMATE) && inst.animation < 0))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "mesh instance refers to an animation outside the array");
    }
    for (uint32_t i = 0; i < d->tri_count; i++) {
        const wpt_tri_geom& g = d->tri_geom[i];
        if ((g.flags & WPT_TRI_ANIMATE) && (g.instance >= d->instance_count || d->instances[g.instance].animation < 0))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "animated triangle without an animated instance");
    }
    for (uint32_t i = 0; i < d->hotspot_count; i++)
        if (d->hotspots[i].animation >= int32_t(d->animation_count))
            return refuse(WPT_ERR_INVALID_ARGUMENT, "hot spot refers to an animation outside the array");
    if (d->envmap.type > WPT_ENV_CUBE)
        return refuse(WPT_ERR_UNSUPPORTED, "environment map type is not known to the kernel");
    if (d->envmap.type == WPT_ENV_EQUIRECT && (d->envmap.tex < 0 || uint32_t(d->envmap.tex) >= d->texture_count))
        return refuse(WPT_ERR_INVALID_ARGUMENT, "environment map references a texture outside the array");
    if (d->envmap.type == WPT_ENV_CUBE) {
        for (int k = 0; k < 6; k++)
            if (d->envmap.cube_tex[k] < 0 || uint32_t(d->envmap.cube_tex[k]) >= d->texture_count)
                return refuse(WPT_ERR_INVALID_ARGUMENT, "environment cube map references a texture outside the array");
    }
    return refuse(WPT_OK, nullptr);
}

/* Storage order of the triangles (triangle index of the caller -> index on the device): that of their leaves in the tree's
 * depth-first order, so that the leaves of a subtree -- which a ray tests one after the other, and neighbouring rays test too --
 * read neighbouring 48-byte records (a 128-byte line holds the triangles of two or three sibling leaves) instead of wherever the
 * meshes' own order put them.  Triangle indices are identities only (leaf -> record, hot spot -> record, the candidate a light
 * ray must end on): no value depends on them.  asGiven (wpt_set_walk(WPT_WALK_TRIANGLES_AS_GIVEN)) keeps the caller's order
 * (measurements). */
inline std::vector<uint32_t> triangleOrder(const wpt_scene_desc* desc, bool asGiven)
{
    const uint32_t n = desc->node_count;
    std::vector<uint32_t> triNew(desc->tri_count, 0xffffffffu);
    uint32_t next = 0;
    if (!asGiven)
        for (uint32_t i = 0; i < n; i++)
            if (desc->nodes[i].kind == WPT_NODE_TRIANGLE && triNew[desc->nodes[i].link] == 0xffffffffu)
                triNew[desc->nodes[i].link] = next++;
    for (uint32_t t = 0; t < desc->tri_count; t++) /* triangles no leaf refers to (or all, in the caller's order) */
        if (triNew[t] == 0xffffffffu)
            triNew[t] = next++;
    return triNew;
}

/* end[i] = first depth-first index behind the subtree of node i (validated) */
inline std::vector<uint32_t> subtreeEnds(const wpt_scene_desc* desc)
{
    const uint32_t n = desc->node_count;
    std::vector<uint32_t> end(n);
    for (uint32_t i = n; i-- > 0;)
        end[i] = desc->nodes[i].kind == WPT_NODE_INNER ? end[desc->nodes[i].link] : i + 1;
    return end;
}

/* Storage order of the nodes (depth-first index -> storage index; place[n] = n ends the walk).  Every ray starts at the root,
 * so the top of the tree is what all waves of an XCD keep fetching; in depth-first order those nodes lie scattered over the
 * whole array (the right child of the root is half the array away), each dragging a 128-byte line of rarely visited neighbours
 * into the XCD's 4 MiB L2.  For trees larger than an L2 the nodes of the top levels are therefore stored first, level by level
 * (topNodes nodes, wpt_set_top_nodes: 2 MiB by default, contiguous and dense), and the subtrees below them after that, each
 * depth-first as before (a walk that descends to a first child then reads the next 32 bytes).  The visiting order is the
 * tree's, not the array's: results do not change. */
inline Status nodePlaces(const wpt_scene_desc* desc, const std::vector<uint32_t>& end, uint32_t topNodes, std::vector<uint32_t>* places)
{
    const uint32_t n = desc->node_count;
    const uint64_t slotCount = n;
    std::vector<uint32_t>& place = *places;
    place.assign(size_t(n) + 1, 0u);
    place[n] = n;
    if (n <= topNodes) /* the whole tree is no larger than the part that would go in front: nothing to gain */
        topNodes = 0;
    uint32_t cursor = 0;
    std::vector<uint32_t> level, next;
    if (topNodes > 0) {
        level.push_back(0);
        while (!level.empty() && cursor + level.size() <= topNodes) {
            next.clear();
            for (uint32_t i : level) {
                place[i] = cursor;
                cursor += 1;
                if (desc->nodes[i].kind == WPT_NODE_INNER) {
                    next.push_back(i + 1);
                    next.push_back(desc->nodes[i].link);
                }
            }
            level.swap(next);
        }
    } else {
        level.push_back(0);
    }
    /* the subtrees that did not make it into the top part, depth-first each, in depth-first order of their roots
     * (blocks of 2 - 6 levels stored level by level instead were measured: 52.3 - 51.8 against 52.7 Msamples/s on the
     * 10 M triangle scene, no difference on the Sponza-class one; locality of the nodes is not what that scene lacks) */
    std::sort(level.begin(), level.end());
    for (uint32_t root : level)
        for (uint32_t i = root; i < end[root]; i++) {
            place[i] = cursor;
            cursor += 1;
        }
    if (cursor != slotCount)
        return refuse(WPT_ERR_INVALID_ARGUMENT, "BVH conversion: the links do not reach every node exactly once");
    return refuse(WPT_OK, nullptr);
}

/* Device node form: two quadwords per node, (lo.x hi.x lo.y lo.z) (hi.y hi.z skip word), in the storage order of nodePlaces
 * with topNodes in front, and one node of padding (kernels that fetch aligned pairs of nodes read the whole last pair).  The
 * reference pops a stack to find the next node after a subtree (bvh.hpp:296,305); in depth-first order that node is the first one
 * behind the subtree, so its place is stored per node ("skip"), an inner node also carries the place of its first child, and the
 * kernel needs neither a stack nor any particular storage order.  word: NODE_CHILD | first child; a triangle's index on the
 * device; PRIM_SPHERE | sphere; an empty node goes where its skip does. */
struct DeviceNodes {
    std::vector<Quad> quads;
    uint32_t boxesMayBeNan;
};

inline Status deviceNodes(const wpt_scene_desc* desc, const std::vector<uint32_t>& triNew, uint32_t topNodes, DeviceNodes* out)
{
    const uint32_t n = desc->node_count;
    out->quads.clear();
    out->boxesMayBeNan = 0u;
    if (n > NODE_INDEX_MASK)
        return refuse(WPT_ERR_UNSUPPORTED, "more than 2^30 - 1 BVH nodes");
    const std::vector<uint32_t> end = subtreeEnds(desc);
    std::vector<uint32_t> place;
    const Status placed = nodePlaces(desc, end, topNodes, &place);
    if (placed.code != WPT_OK)
        return placed;
    /* a local array and flag, handed over at the end: filled through `out` the loop reloads them, 4 % of a 1 M triangle scene's
     * upload (profiles/scene_layout_upload_ab.txt) */
    std::vector<Quad> dev(size_t(n) * 2 + 2, quad(0.0f, 0.0f, 0.0f, 0.0f));
    uint32_t boxesMayBeNan = 0u;
    for (uint32_t i = 0; i < n; i++) {
        const wpt_bvh_node& nd = desc->nodes[i];
        const uint32_t skip = place[end[i]];
        const uint32_t word = nd.kind == WPT_NODE_INNER ? (NODE_CHILD | place[i + 1]) : nd.kind == WPT_NODE_TRIANGLE ? triNew[nd.link]
            : nd.kind == WPT_NODE_SPHERE ? (PRIM_SPHERE | nd.link) : (NODE_CHILD | skip);
        float sk, wd;
        memcpy(&sk, &skip, 4);
        memcpy(&wd, &word, 4);
        dev[2 * size_t(place[i])] = quad(nd.lo[0], nd.hi[0], nd.lo[1], nd.lo[2]); /* nodeLo / nodeHi (wpt_device.h) */
        dev[2 * size_t(place[i]) + 1] = quad(nd.hi[1], nd.hi[2], sk, wd);
        for (int a = 0; a < 3; a++)
            if (nd.lo[a] != nd.lo[a] || nd.hi[a] != nd.hi[a])
                boxesMayBeNan = 1u;
    }
    out->quads.swap(dev);
    out->boxesMayBeNan = boxesMayBeNan;
    return refuse(WPT_OK, nullptr);
}

/* Nodes whose link the LDS copy of a tree folds (wpt_fold.h: they go past one or more first children with their own box),
 * counted with the rule the kernels' prologue applies over device nodes (8 words each) in the order the kernels see them.
 * words (or NULL): every node's word 7 in LDS. */
inline uint32_t countFoldedLinks(const uint32_t* nodes, uint32_t nodeCount, uint32_t* words)
{
    uint32_t folded = 0;
    for (uint32_t i = 0; i < nodeCount; i++) {
        uint32_t links;
        const uint32_t word = wptf::foldLdsWord(nodes, nodeCount, i, true, &links);
        folded += links > 0 ? 1u : 0u;
        if (words)
            words[i] = word;
    }
    return folded;
}

/* Ordered box copies (the 1024-lane kernels with the scene in LDS, wpt_pathtrace.inc.h): the node array of a tree that fits LDS
 * once per sign octant of a ray's direction, eight copies of 2 * nodeCount + 2 quadwords one behind the other.  Copy k has bit a
 * set for a negative axis a, and on such an axis a record holds (-hi, -lo) in the places of (lo, hi): a ray that walks with that
 * axis mirrored (origin and reciprocal negated) finds the near bound where lo stands and the far bound where hi stands on every
 * axis, so that its box test sorts nothing.  Negation is exact, so the six slab distances are the ones the ray computes from the
 * plain record, bit for bit.  Links and words are copied as they are, and so is the padding behind the last node, where the
 * kernels put their null node; copy 0 is deviceNodes' array byte for byte.  `nodes`: device nodes, eight words each (the padding
 * node is added here).  The argument needs lo <= hi on every axis of every node, which a NaN bound fails too: such a tree has no
 * ordered copies (false, *out empty) and is walked from the plain record. */
constexpr uint32_t ORDERED_COPIES = 8;

inline bool orderedBoxCopies(const uint32_t* nodes, uint32_t nodeCount, std::vector<Quad>* out)
{
    out->clear();
    std::vector<Quad> plain(2 * size_t(nodeCount) + 2, quad(0.0f, 0.0f, 0.0f, 0.0f));
    if (nodeCount > 0)
        memcpy(plain.data(), nodes, 2 * size_t(nodeCount) * sizeof(Quad));
    for (uint32_t i = 0; i < nodeCount; i++) {
        const Quad &q0 = plain[2 * size_t(i)], &q1 = plain[2 * size_t(i) + 1];
        if (!(q0.x <= q0.y && q0.z <= q1.x && q0.w <= q1.y))
            return false;
    }
    std::vector<Quad> copies;
    copies.reserve(ORDERED_COPIES * plain.size());
    for (uint32_t k = 0; k < ORDERED_COPIES; k++)
        for (uint32_t i = 0; i <= nodeCount; i++) {
            Quad q0 = plain[2 * size_t(i)], q1 = plain[2 * size_t(i) + 1];
            if (i < nodeCount) {
                if (k & 1u) {
                    const float lo = q0.x;
                    q0.x = -q0.y;
                    q0.y = -lo;
                }
                if (k & 2u) {
                    const float lo = q0.z;
                    q0.z = -q1.x;
                    q1.x = -lo;
                }
                if (k & 4u) {
                    const float lo = q0.w;
                    q0.w = -q1.y;
                    q1.y = -lo;
                }
            }
            copies.push_back(q0);
            copies.push_back(q1);
        }
    out->swap(copies);
    return true;
}

/* Where those copies lie in a compute unit's LDS, and which parts of a hit's data -- a record per triangle, the hot spots, the
 * instances' normal matrices -- follow them there in front of the paths' cold words: wptk::orderedPlaces and
 * wptk::hitDataPlaces of wpt_lds_places.h (included above), pure functions of the scene's counts that the launch and the
 * kernels both ask.  The instance count they are given is this one: the normal matrix is read for a triangle with
 * WPT_TRI_TRANSFORM only, so the matrices in LDS are those of instances 0 .. the largest one such a triangle names; 0 where no
 * triangle is transformed. */
inline uint32_t normalsNamed(const wpt_scene_desc* desc)
{
    uint32_t named = 0;
    for (uint32_t i = 0; i < desc->tri_count; i++)
        if ((desc->tri_geom[i].flags & WPT_TRI_TRANSFORM) && desc->tri_geom[i].instance >= named)
            named = desc->tri_geom[i].instance + 1;
    return named;
}

/* The wide form (wpt_pathtrace.inc.h): the binary tree collapsed by one level, eight quadwords per wide node (lo.x lo.y lo.z
 * hi.x hi.y hi.z of the up to four entries, their references, one spare).  Wide nodes are made for the root and for every inner
 * node that is an entry of a wide node, in depth-first order (a wide node's first inner entry follows it).  The walk's argument
 * needs finite boxes and every child's box within its parent's; its stack needs the tree's worst case to fit.  A tree that fails
 * any of the three has no wide form (an empty result) and is walked as it is.  *worstStack (or NULL): the entries the walk can
 * have pending at once, 0xffffffff where the boxes already rule the form out. */
inline std::vector<Quad> wideNodes(const wpt_scene_desc* desc, const std::vector<uint32_t>& triNew, uint32_t* worstStack = nullptr)
{
    const uint32_t n = desc->node_count;
    if (worstStack)
        *worstStack = 0xffffffffu;
    bool ok = true;
    for (uint32_t i = 0; i < n && ok; i++) {
        const wpt_bvh_node& nd = desc->nodes[i];
        for (int a = 0; a < 3; a++)
            ok = ok && std::isfinite(nd.lo[a]) && std::isfinite(nd.hi[a]);
        if (nd.kind == WPT_NODE_INNER) {
            const uint32_t child[2] = { i + 1, nd.link };
            for (int k = 0; k < 2; k++)
                for (int a = 0; a < 3; a++)
                    ok = ok && desc->nodes[child[k]].lo[a] >= nd.lo[a] && desc->nodes[child[k]].hi[a] <= nd.hi[a];
        }
    }
    std::vector<Quad> wide;
    std::vector<uint32_t> made;        /* binary node of each wide node, in order of creation */
    std::vector<uint32_t> entries;     /* 4 per wide node: binary nodes, 0xffffffff = none */
    if (ok) {
        std::vector<uint32_t> todo(1, 0u); /* depth first: a stack of binary nodes to make wide nodes for */
        while (!todo.empty()) {
            const uint32_t x = todo.back();
            todo.pop_back();
            made.push_back(x);
            uint32_t entry[4] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu };
            int count = 0;
            if (desc->nodes[x].kind == WPT_NODE_INNER) {
                const uint32_t child[2] = { x + 1, desc->nodes[x].link };
                for (int k = 0; k < 2; k++) {
                    if (desc->nodes[child[k]].kind == WPT_NODE_INNER) {
                        entry[count++] = child[k] + 1;
                        entry[count++] = desc->nodes[child[k]].link;
                    } else {
                        entry[count++] = child[k];
                    }
                }
            } else {
                entry[count++] = x; /* a tree of one leaf */
            }
            for (int k = 0; k < 4; k++)
                entries.push_back(entry[k]);
            for (int k = count - 1; k >= 0; k--) /* the first inner entry is made next */
                if (desc->nodes[entry[k]].kind == WPT_NODE_INNER && entry[k] != x)
                    todo.push_back(entry[k]);
        }
        ok = made.size() <= NODE_INDEX_MASK;
    }
    if (ok) {
        /* wide index of every binary node that has one; creation order is a pre-order, so a reverse pass sees children first */
        std::vector<uint32_t> wideOf(n, 0xffffffffu);
        for (size_t w = 0; w < made.size(); w++)
            wideOf[made[w]] = uint32_t(w);
        std::vector<uint32_t> depth(made.size(), 0u); /* entries that can wait on the stack while the walk is below this wide node */
        for (size_t w = made.size(); w-- > 0;) {
            int count = 0;
            while (count < 4 && entries[4 * w + count] != 0xffffffffu)
                count++;
            uint32_t worst = 0;
            for (int k = 0; k < count; k++) {
                const uint32_t e = entries[4 * w + k];
                const uint32_t below = (desc->nodes[e].kind == WPT_NODE_INNER && e != made[w]) ? depth[wideOf[e]] : 0u;
                worst = std::max(worst, uint32_t(count - 1 - k) + below);
            }
            depth[w] = worst;
        }
        if (worstStack)
            *worstStack = depth[0];
        ok = depth[0] <= WIDE_STACK;
        wide.resize(made.size() * 8, quad(0.0f, 0.0f, 0.0f, 0.0f));
        for (size_t w = 0; w < made.size() && ok; w++) {
            float q[8][4];
            uint32_t ref[4] = { WIDE_NONE, WIDE_NONE, WIDE_NONE, WIDE_NONE };
            for (int r = 0; r < 8; r++)
                for (int k = 0; k < 4; k++)
                    q[r][k] = 0.0f;
            for (int k = 0; k < 4; k++) {
                const uint32_t e = entries[4 * w + k];
                if (e == 0xffffffffu)
                    continue;
                const wpt_bvh_node& nd = desc->nodes[e];
                for (int a = 0; a < 3; a++) {
                    q[a][k] = nd.lo[a];
                    q[3 + a][k] = nd.hi[a];
                }
                if (nd.kind == WPT_NODE_INNER)
                    ref[k] = NODE_CHILD | wideOf[e];
                else if (nd.kind == WPT_NODE_TRIANGLE)
                    ref[k] = triNew[nd.link];
                else if (nd.kind == WPT_NODE_SPHERE)
                    ref[k] = PRIM_SPHERE | nd.link;
            }
            memcpy(q[6], ref, 16);
            for (int r = 0; r < 8; r++)
                wide[8 * w + r] = quad(q[r][0], q[r][1], q[r][2], q[r][3]);
        }
    }
    if (!ok)
        wide.clear();
    return wide;
}

/* the per-triangle records (wpt_tri_geom, wpt_tri_attr) in the device's triangle order */
template<typename T> std::vector<T> permuted(const T* records, const std::vector<uint32_t>& triNew)
{
    std::vector<T> r(triNew.size());
    for (size_t t = 0; t < triNew.size(); t++)
        r[triNew[t]] = records[t];
    return r;
}

/* the hot spots with a triangle's index on the device; a sphere's is the caller's */
inline std::vector<wpt_hotspot> remappedHotspots(const wpt_scene_desc* desc, const std::vector<uint32_t>& triNew)
{
    std::vector<wpt_hotspot> h(desc->hotspots, desc->hotspots + desc->hotspot_count);
    for (wpt_hotspot& hs : h)
        if (hs.kind != WPT_HOTSPOT_SPHERE)
            hs.prim = triNew[hs.prim];
    return h;
}

/* Image textures are decoded once, at the upload, into one pool of RGBA float4 texels (16 bytes per texel whatever the file
 * format was: HBM is large, instructions per lookup are not); the device copies of the texture records index that pool: an
 * image's texel_offset counts texels of the pool.  *texelCount: the pool's size. */
inline std::vector<wpt_texture> texelOffsets(const wpt_scene_desc* desc, size_t* texelCount)
{
    std::vector<wpt_texture> devTex(desc->textures, desc->textures + desc->texture_count);
    *texelCount = 0;
    for (wpt_texture& t : devTex) {
        if (t.type == WPT_TEX_IMAGE) {
            t.texel_offset = *texelCount;
            *texelCount += size_t(t.width) * t.height;
        }
    }
    return devTex;
}

/* The measured BRDFs' pool, and behind it one interleaved table per BRDF whose colour and luminance warps share their grids
 * (wpt_rgl.h, rglColourInterleaved): red, green, blue and luminance of a grid point side by side, so that the up to 128 look-ups
 * an evaluation makes into those two warps come from 8 cache lines instead of 32.  The values are the pool's own; which copy a
 * look-up reads changes no bit.  rgbl: per BRDF, where its table starts in the pool (in floats), WPT_RGL_NONE without one. */
struct RglPool {
    std::vector<float> pool;
    std::vector<uint32_t> rgbl;
};

inline RglPool rglPool(const wpt_scene_desc* desc)
{
    RglPool r;
    std::vector<float>& pool = r.pool;
    std::vector<uint32_t>& rgbl = r.rgbl;
    pool.assign(desc->rgl_data, desc->rgl_data + desc->rgl_data_count);
    rgbl.assign(desc->rgl_count, WPT_RGL_NONE);
    for (uint32_t i = 0; i < desc->rgl_count; i++) {
        const wpt_rgl_brdf& b = desc->rgl_brdfs[i];
        if (!wptrgl::rglInterleavable(b))
            continue;
        const size_t size = size_t(b.rgb.size_x) * b.rgb.size_y;
        const size_t slices = size_t(b.luminance.param_size[0]) * b.luminance.param_size[1];
        const size_t at = (pool.size() + 3) & ~size_t(3); /* 16-byte records */
        if (at + slices * size * 4 > 0xfffffff0ull)
            continue;
        pool.resize(at + slices * size * 4);
        for (size_t sl = 0; sl < slices; sl++)
            for (size_t e = 0; e < size; e++) {
                float* t = pool.data() + at + (sl * size + e) * 4;
                for (size_t c = 0; c < 3; c++)
                    t[c] = desc->rgl_data[b.rgb.data + (sl * 3 + c) * size + e];
                t[3] = desc->rgl_data[b.luminance.data + sl * size + e];
            }
        rgbl[i] = uint32_t(at);
    }
    return r;
}

/* EnvironmentMap::initializeImportanceSampling (envmap.hpp:121-158) from the per-bin importance: sum, sort and prefix sum in
 * the reference's sequential order.  M: the importance normalised; Ms: the bins by descending M; Mcs: the running sum in that order. */
struct EnvTables {
    std::vector<float> M, Mcs;
    std::vector<int32_t> Ms;
};

inline EnvTables envTablesFromImportance(const float* importance, size_t bins)
{
    EnvTables t;
    t.M.assign(importance, importance + bins);
    float total = 0.0f;
    for (size_t i = 0; i < bins; i++)
        total += t.M[i];
    for (size_t i = 0; i < bins; i++)
        t.M[i] /= total;
    t.Ms.resize(bins);
    for (size_t i = 0; i < bins; i++)
        t.Ms[i] = int32_t(i);
    const std::vector<float>& M = t.M;
    std::sort(t.Ms.begin(), t.Ms.end(), [&M](unsigned int i, unsigned int j) { return M[i] > M[j]; });
    t.Mcs.resize(bins);
    float sum = 0.0f;
    for (size_t i = 0; i < bins; i++) {
        sum += M[t.Ms[i]];
        t.Mcs[i] = sum;
    }
    return t;
}

/* start table for the sampling search (envD in wpt_device.h): ENV_LUT_SIZE + 1 entries, lut[k] = the first bin whose cumulative
 * value reaches k / ENV_LUT_SIZE.  Only for a non-decreasing cumulative table, which is what the construction gives -- a caller's
 * own table that is not gets none (an empty result) and the plain bisection. */
constexpr uint32_t ENV_LUT_SIZE = 65536;

inline std::vector<int32_t> envStartTable(const float* Mcs, size_t bins)
{
    std::vector<int32_t> lut;
    bool monotone = true;
    for (size_t i = 1; i < bins && monotone; i++)
        monotone = !(Mcs[i] < Mcs[i - 1]);
    if (monotone) {
        const uint32_t K = ENV_LUT_SIZE;
        lut.resize(K + 1);
        size_t i = 0;
        for (uint32_t k = 0; k < K; k++) {
            const float t = float(k) / float(K);
            while (i < bins && Mcs[i] < t)
                i++;
            lut[k] = int32_t(i < bins ? i : bins - 1);
        }
        lut[K] = int32_t(bins - 1);
    }
    return lut;
}

/* log2 of a power of two, else -1 */
inline int envLog2(int N)
{
    int log2N = -1;
    if (N > 0 && (N & (N - 1)) == 0)
        for (int b = 0; b < 31; b++)
            if ((1 << b) == N)
                log2N = b;
    return log2N;
}

} // namespace wptl

#endif
