/* scene_layout_check.cpp -- the functions of wurblpt_amd/csrc/wpt_scene_layout.h on their own, built with
 * -fsanitize=address,undefined by tests/test_scene_layout.py and run as a program.
 *
 * Makes seeded random descriptions -- a binary tree in the reference's depth-first form over T triangles with sphere leaves and
 * empty nodes, leaves that share a triangle and triangles no leaf refers to, triangle and sphere hot spots, image and other
 * textures, two synthetic measured-BRDF descriptors of which one can be interleaved -- lays each out with 0, 1, 2, 3, 7, n - 1,
 * n, n + 1 and 65536 nodes in front and both triangle orders, and checks what must hold of the arrays whatever the
 * implementation: the storage order, the links (a stackless walk over the quadwords sees the description's leaves in its
 * depth-first order), boxesMayBeNan, the triangle permutation and what moved with it, the wide form (its expansion, its bounds,
 * its stack's worst case against a simulated walk, and the three reasons not to offer it), the texel offsets, the measured
 * BRDFs' tables, the environment's tables and start table.  Then damages valid descriptions at random (indices, links, kinds,
 * counts, offsets; never a pointer or an array's length) and runs every layout function over what validate() still accepts:
 * the sanitizers see every index the layout follows.
 *
 * Prints one summary line; exit status 1 if a rule is broken.  With --digests: a 64-bit FNV-1a of every array for six fixed
 * seeds, which tests/golden/scene_layout_digests.json pins. */
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_scene_layout.h"

using namespace wptl;

static long failures = 0;
static long checksRun = 0;

static void check(bool ok, const char* rule, uint64_t seed, uint32_t top, int asGiven)
{
    checksRun++;
    if (ok)
        return;
    if (failures++ < 30)
        printf("BROKEN %s: seed %" PRIu64 " nodes in front %u triangles %s\n", rule, seed, top, asGiven ? "as given" : "by leaves");
}

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull) {}
    uint64_t next()
    {
        s += 0x9e3779b97f4a7c15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return n ? uint32_t(next() % n) : 0u; }
    float unit() { return float(next() >> 40) / float(1 << 24); }
};

static uint32_t bitsOf(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

/* a description and the arrays it points into */
struct Scene {
    std::vector<wpt_bvh_node> nodes;
    std::vector<wpt_tri_geom> geom;
    std::vector<wpt_tri_attr> attr;
    std::vector<wpt_instance> instances;
    std::vector<wpt_material> materials;
    std::vector<wpt_texture> textures;
    std::vector<uint8_t> texels;
    std::vector<wpt_hotspot> hotspots;
    std::vector<wpt_sphere> spheres;
    std::vector<wpt_rgl_brdf> brdfs;
    std::vector<float> rglData;
    std::vector<wpt_animation> animations;
    std::vector<wpt_keyframe> keyframes;
    wpt_scene_desc d;

    void point()
    {
        memset(&d, 0, sizeof(d));
        d.abi_version = WPT_ABI_VERSION;
        d.node_count = uint32_t(nodes.size());
        d.tri_count = uint32_t(geom.size());
        d.instance_count = uint32_t(instances.size());
        d.material_count = uint32_t(materials.size());
        d.texture_count = uint32_t(textures.size());
        d.hotspot_count = uint32_t(hotspots.size());
        d.sphere_count = uint32_t(spheres.size());
        d.texel_bytes = texels.size();
        d.nodes = nodes.data();
        d.tri_geom = geom.data();
        d.tri_attr = attr.data();
        d.instances = instances.data();
        d.materials = materials.data();
        d.textures = textures.data();
        d.texels = texels.data();
        d.hotspots = hotspots.data();
        d.spheres = spheres.data();
        d.rgl_count = uint32_t(brdfs.size());
        d.rgl_data_count = rglData.size();
        d.rgl_brdfs = brdfs.data();
        d.rgl_data = rglData.data();
        d.animation_count = uint32_t(animations.size());
        d.keyframe_count = uint32_t(keyframes.size());
        d.animations = animations.data();
        d.keyframes = keyframes.data();
        d.envmap.type = WPT_ENV_NONE;
        d.envmap.tex = -1;
        for (int k = 0; k < 6; k++)
            d.envmap.cube_tex[k] = -1;
    }
};

struct Leaf {
    uint32_t kind, prim;
    float lo[3], hi[3];
};

/* the leaves' subtree in the reference's depth-first form: an inner node, its first child's subtree, its second child's (link);
 * an inner node's box is the union of its children's (exactly: no arithmetic) */
static void buildTree(Rng& rng, const std::vector<Leaf>& leaves, size_t first, size_t count, std::vector<wpt_bvh_node>& out)
{
    wpt_bvh_node nd;
    memset(&nd, 0, sizeof(nd));
    if (count == 1) {
        const Leaf& l = leaves[first];
        nd.kind = l.kind;
        nd.link = l.prim;
        for (int a = 0; a < 3; a++) {
            nd.lo[a] = l.lo[a];
            nd.hi[a] = l.hi[a];
        }
        out.push_back(nd);
        return;
    }
    /* mostly near the middle, sometimes lopsided: depth stays far below the recursion's limits */
    size_t left = rng.below(4) ? count / 2 + rng.below(uint32_t(count / 4 + 1)) - count / 8 : 1 + rng.below(uint32_t(count - 1));
    left = left < 1 ? 1 : left > count - 1 ? count - 1 : left;
    const size_t self = out.size();
    nd.kind = WPT_NODE_INNER;
    out.push_back(nd);
    buildTree(rng, leaves, first, left, out);
    const uint32_t link = uint32_t(out.size());
    buildTree(rng, leaves, first + left, count - left, out);
    out[self].link = link;
    for (int a = 0; a < 3; a++) {
        out[self].lo[a] = std::min(out[self + 1].lo[a], out[link].lo[a]);
        out[self].hi[a] = std::max(out[self + 1].hi[a], out[link].hi[a]);
    }
}

/* one warp of a measured BRDF with its grids and tables in the pool */
static wpt_rgl_warp makeWarp(Rng& rng, std::vector<float>& pool, uint32_t dims, uint32_t sx, uint32_t sy, const uint32_t* psize, const uint32_t* pstride, bool cdf)
{
    auto alloc = [&](size_t n) {
        const size_t at = pool.size();
        for (size_t i = 0; i < n; i++)
            pool.push_back(rng.unit());
        return uint32_t(at);
    };
    wpt_rgl_warp w;
    memset(&w, 0, sizeof(w));
    w.size_x = sx;
    w.size_y = sy;
    w.dims = dims;
    size_t slices = 1;
    for (uint32_t k = 0; k < dims; k++) {
        w.param_size[k] = psize[k];
        w.param_stride[k] = pstride[k];
        w.param_values[k] = alloc(psize[k]);
        slices *= psize[k];
    }
    w.data = alloc(slices * sx * sy);
    w.marginal_cdf = cdf ? alloc(slices * sy) : WPT_RGL_NONE;
    w.conditional_cdf = cdf ? alloc(slices * sx * sy) : WPT_RGL_NONE;
    return w;
}

static wpt_rgl_brdf makeBrdf(Rng& rng, std::vector<float>& pool, bool interleavable)
{
    const uint32_t p0 = 1 + rng.below(3), p1 = 1 + rng.below(3), sx = 2 + rng.below(3), sy = 2 + rng.below(3);
    const uint32_t two[2] = { p0, p1 }, twoStride[2] = { p1, 1 };
    const uint32_t three[3] = { p0, p1, 3 }, threeStride[3] = { 3 * p1, 3, 1 };
    wpt_rgl_brdf b;
    memset(&b, 0, sizeof(b));
    uint32_t size[6]; /* drawn in order: the order of a call's arguments is the compiler's */
    for (uint32_t& v : size)
        v = 2 + rng.below(3);
    b.ndf = makeWarp(rng, pool, 0, size[0], size[1], nullptr, nullptr, false);
    b.sigma = makeWarp(rng, pool, 0, size[2], size[3], nullptr, nullptr, false);
    b.vndf = makeWarp(rng, pool, 2, size[4], size[5], two, twoStride, true);
    b.luminance = makeWarp(rng, pool, 2, sx, sy, two, twoStride, true);
    b.rgb = makeWarp(rng, pool, 3, interleavable ? sx : sx + 1, sy, three, threeStride, false); /* another grid: no shared table */
    b.isotropic = 1;
    return b;
}

static Scene makeScene(uint64_t seed, uint32_t T)
{
    Rng rng(seed);
    Scene s;
    /* triangles: a third of them have no leaf; the others have one, and some a second or third */
    s.geom.resize(T);
    s.attr.resize(T);
    for (uint32_t t = 0; t < T; t++) {
        memset(&s.geom[t], 0, sizeof(wpt_tri_geom));
        memset(&s.attr[t], 0, sizeof(wpt_tri_attr));
        s.geom[t].v0[0] = float(t); /* the record's own name: it must move with its index */
        s.geom[t].v1[1] = rng.unit();
        s.geom[t].instance = rng.below(2);
        s.geom[t].material = rng.below(3);
        s.attr[t].n0[0] = float(t);
        s.attr[t].t2[2] = rng.unit();
    }
    const uint32_t sphereCount = 1 + rng.below(4);
    std::vector<Leaf> leaves;
    auto leaf = [&](uint32_t kind, uint32_t prim) {
        Leaf l;
        l.kind = kind;
        l.prim = prim;
        for (int a = 0; a < 3; a++) {
            l.lo[a] = rng.unit() * 10.0f - 5.0f;
            l.hi[a] = l.lo[a] + rng.unit();
        }
        leaves.push_back(l);
    };
    for (uint32_t t = 0; t < T; t++)
        if (T < 3 || rng.below(3)) {
            const bool second = rng.below(5) == 0, third = rng.below(11) == 0;
            for (int copies = 1 + second + third; copies > 0; copies--)
                leaf(WPT_NODE_TRIANGLE, t);
        }
    for (uint32_t k = 0; k < sphereCount; k++)
        leaf(WPT_NODE_SPHERE, rng.below(sphereCount));
    for (uint32_t k = rng.below(4); k > 0; k--)
        leaf(WPT_NODE_EMPTY, 0);
    for (size_t i = leaves.size(); i > 1; i--) /* the leaves in any order */
        std::swap(leaves[i - 1], leaves[rng.below(uint32_t(i))]);
    buildTree(rng, leaves, 0, leaves.size(), s.nodes);

    s.instances.resize(2);
    memset(s.instances.data(), 0, 2 * sizeof(wpt_instance));
    s.instances[0].animation = -1;
    s.instances[1].animation = 0;
    s.materials.resize(4);
    memset(s.materials.data(), 0, 4 * sizeof(wpt_material));
    for (uint32_t m = 0; m < 4; m++) {
        s.materials[m].type = m == 3 ? WPT_MAT_RGL : m == 2 ? WPT_MAT_LIGHT_DIFFUSE : WPT_MAT_LAMBERTIAN;
        s.materials[m].normal_tex = -1;
        for (int k = 0; k < 5; k++)
            s.materials[m].tex[k] = -1;
    }
    s.materials[0].tex[0] = 1;
    s.materials[3].tex[0] = int32_t(rng.below(2));
    /* textures: constant, image, checker, image, transformer of an image, image */
    const uint32_t types[6] = { WPT_TEX_CONSTANT, WPT_TEX_IMAGE, WPT_TEX_CHECKER, WPT_TEX_IMAGE, WPT_TEX_TRANSFORMER, WPT_TEX_IMAGE };
    for (uint32_t k = 0; k < 6; k++) {
        wpt_texture t;
        memset(&t, 0, sizeof(t));
        t.type = types[k];
        t.child = t.type == WPT_TEX_TRANSFORMER ? 3 : -1;
        t.width = 1 + rng.below(5);
        t.height = 1 + rng.below(5);
        if (t.type == WPT_TEX_IMAGE) {
            t.comps = 1 + rng.below(4);
            t.texel_type = rng.below(3);
            const size_t bytes = size_t(t.width) * t.height * t.comps * (t.texel_type == WPT_TEXEL_U8 ? 1 : t.texel_type == WPT_TEXEL_U16 ? 2 : 4);
            t.texel_offset = s.texels.size() + rng.below(3); /* the caller's pool need not be dense */
            s.texels.resize(size_t(t.texel_offset) + bytes, uint8_t(k));
        } else {
            t.texel_offset = 1000 + k; /* not an image: the word is the caller's and stays */
        }
        s.textures.push_back(t);
    }
    s.spheres.resize(sphereCount);
    memset(s.spheres.data(), 0, sphereCount * sizeof(wpt_sphere));
    for (wpt_sphere& sp : s.spheres) {
        sp.radius = 1.0f;
        sp.material = rng.below(3);
        sp.animation = rng.below(2) ? -1 : 1;
    }
    for (uint32_t k = 1 + rng.below(5); k > 0; k--) {
        wpt_hotspot h;
        memset(&h, 0, sizeof(h));
        h.kind = rng.below(3) ? WPT_HOTSPOT_TRIANGLE : WPT_HOTSPOT_SPHERE;
        h.prim = h.kind == WPT_HOTSPOT_SPHERE ? rng.below(sphereCount) : rng.below(T);
        h.animation = -1;
        h.p0[0] = float(s.hotspots.size());
        s.hotspots.push_back(h);
    }
    s.brdfs.push_back(makeBrdf(rng, s.rglData, true));
    for (uint32_t pad = rng.below(4); pad > 0; pad--) /* tables end anywhere: an interleaved one still starts on a 16-byte record */
        s.rglData.push_back(rng.unit());
    s.brdfs.push_back(makeBrdf(rng, s.rglData, false));
    if (rng.below(2))
        std::swap(s.brdfs[0], s.brdfs[1]);
    for (uint32_t a = 0; a < 2; a++) {
        wpt_animation an = { uint32_t(s.keyframes.size()), 2 + rng.below(2) };
        for (uint32_t k = 0; k < an.keyframe_count; k++) {
            wpt_keyframe kf;
            memset(&kf, 0, sizeof(kf));
            kf.t = float(k);
            kf.rotation[3] = 1.0f;
            s.keyframes.push_back(kf);
        }
        s.animations.push_back(an);
    }
    s.point();
    return s;
}

/* what the description says, found without the layout's own passes: a descent from the root over child links */
struct Tree {
    std::vector<uint32_t> depth, size, parent;
    std::vector<uint32_t> leaves; /* triangle and sphere leaves in depth-first order */
    bool anyNan;
};

static Tree readTree(const Scene& s)
{
    const uint32_t n = s.d.node_count;
    Tree t;
    t.depth.assign(n, 0);
    t.size.assign(n, 1);
    t.parent.assign(n, 0xffffffffu);
    t.anyNan = false;
    std::vector<uint32_t> stack(1, 0u), order;
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        order.push_back(i);
        const wpt_bvh_node& nd = s.nodes[i];
        for (int a = 0; a < 3; a++)
            t.anyNan = t.anyNan || std::isnan(nd.lo[a]) || std::isnan(nd.hi[a]);
        if (nd.kind == WPT_NODE_INNER) {
            const uint32_t child[2] = { nd.link, i + 1 };
            for (uint32_t c : child) {
                t.depth[c] = t.depth[i] + 1;
                t.parent[c] = i;
                stack.push_back(c);
            }
        } else if (nd.kind != WPT_NODE_EMPTY) {
            t.leaves.push_back(i);
        }
    }
    for (size_t k = order.size(); k-- > 1;)
        t.size[t.parent[order[k]]] += t.size[order[k]];
    return t;
}

/* word k of record `index` of `words` 32-bit words each */
static uint32_t wordOf(const std::vector<Quad>& q, size_t index, size_t words, size_t k)
{
    uint32_t u;
    memcpy(&u, reinterpret_cast<const unsigned char*>(q.data()) + 4 * (index * words + k), 4);
    return u;
}

static uint32_t word(const std::vector<Quad>& q, size_t slot, int k)
{
    return wordOf(q, slot, 8, size_t(k));
}

static void checkNodes(const Scene& s, const Tree& tree, const std::vector<uint32_t>& triNew, uint32_t top, uint64_t seed, int asGiven)
{
    const uint32_t n = s.d.node_count;
    auto rule = [&](bool ok, const char* what) { check(ok, what, seed, top, asGiven); };
    std::vector<uint32_t> place;
    const Status placed = nodePlaces(&s.d, subtreeEnds(&s.d), top, &place);
    DeviceNodes dn;
    const Status st = deviceNodes(&s.d, triNew, top, &dn);
    rule(placed.code == WPT_OK && st.code == WPT_OK && place.size() == size_t(n) + 1 && dn.quads.size() == size_t(n) * 2 + 2, "a valid tree has device nodes");
    if (placed.code != WPT_OK || st.code != WPT_OK || place.size() != size_t(n) + 1 || dn.quads.size() != size_t(n) * 2 + 2)
        return;
    /* storage order */
    std::vector<uint32_t> inv(n, 0xffffffffu);
    bool perm = place[n] == n;
    for (uint32_t i = 0; i < n && perm; i++) {
        perm = place[i] < n && inv[place[i]] == 0xffffffffu;
        if (perm)
            inv[place[i]] = i;
    }
    rule(perm && place[0] == 0, "place is a permutation with the root at 0");
    if (!perm)
        return;
    if (top == 0 || n <= top) {
        bool identity = true;
        for (uint32_t i = 0; i < n; i++)
            identity = identity && place[i] == i;
        rule(identity, "nothing in front: the depth-first order");
    } else {
        /* whole levels while they fit: the nodes in front are those above the first level that does not */
        std::vector<uint32_t> perLevel;
        for (uint32_t i = 0; i < n; i++) {
            if (tree.depth[i] >= perLevel.size())
                perLevel.resize(tree.depth[i] + 1, 0u);
            perLevel[tree.depth[i]]++;
        }
        uint32_t front = 0, levels = 0;
        while (levels < perLevel.size() && front + perLevel[levels] <= top)
            front += perLevel[levels++];
        rule(front <= top, "the nodes in front number at most topNodes");
        bool byLevel = true, frontIsTop = true;
        for (uint32_t slot = 0; slot < front; slot++) {
            frontIsTop = frontIsTop && tree.depth[inv[slot]] < levels;
            byLevel = byLevel && (slot == 0 || tree.depth[inv[slot - 1]] <= tree.depth[inv[slot]]);
        }
        rule(frontIsTop, "in front are the top levels");
        rule(byLevel, "level by level: depths in front never decrease");
        bool contiguous = true;
        uint32_t cursor = front;
        for (uint32_t i = 0; i < n; i++)
            if (tree.depth[i] == levels) { /* the roots of the subtrees behind, in depth-first order */
                for (uint32_t j = 0; j < tree.size[i]; j++)
                    contiguous = contiguous && place[i + j] == cursor + j;
                cursor += tree.size[i];
            }
        rule(contiguous && cursor == n, "every subtree behind is contiguous and depth-first");
    }
    /* links */
    bool skips = true, boxes = true, words = true;
    for (uint32_t i = 0; i < n; i++) {
        const wpt_bvh_node& nd = s.nodes[i];
        const size_t slot = place[i];
        const float want[6] = { nd.lo[0], nd.hi[0], nd.lo[1], nd.lo[2], nd.hi[1], nd.hi[2] };
        for (int k = 0; k < 6; k++)
            boxes = boxes && word(dn.quads, slot, k) == bitsOf(want[k]);
        const uint32_t behind = i + tree.size[i]; /* first depth-first node behind the subtree */
        skips = skips && word(dn.quads, slot, 6) == place[behind];
        const uint32_t w = word(dn.quads, slot, 7);
        if (nd.kind == WPT_NODE_INNER)
            words = words && w == (NODE_CHILD | place[i + 1]);
        else if (nd.kind == WPT_NODE_TRIANGLE)
            words = words && w == triNew[nd.link] && w < PRIM_SPHERE;
        else if (nd.kind == WPT_NODE_SPHERE)
            words = words && w == (PRIM_SPHERE | nd.link) && w < NODE_CHILD;
        else
            words = words && w == (NODE_CHILD | place[behind]);
    }
    rule(boxes, "six bounds: the description's bits in the record's word order");
    rule(skips, "skip: the place of the first depth-first node behind the subtree");
    rule(words, "word: first child, remapped triangle, sphere, or an empty node's way out");
    /* the stackless walk that enters every inner node */
    uint32_t slot = 0, steps = 0;
    size_t seen = 0;
    bool walk = true;
    while (slot != n && steps <= n && walk) {
        walk = slot < n && inv[slot] == steps; /* the visiting order is the tree's, whatever the array's */
        if (!walk)
            break;
        steps++;
        const uint32_t w = word(dn.quads, slot, 7);
        if (w >= NODE_CHILD) {
            slot = w & NODE_INDEX_MASK;
        } else {
            const wpt_bvh_node& nd = s.nodes[seen < tree.leaves.size() ? tree.leaves[seen] : 0];
            walk = seen < tree.leaves.size() && (w & PRIM_SPHERE ? nd.kind == WPT_NODE_SPHERE && (w & ~PRIM_SPHERE) == nd.link
                    : nd.kind == WPT_NODE_TRIANGLE && w == triNew[nd.link]);
            seen++;
            slot = word(dn.quads, slot, 6);
        }
    }
    rule(walk && slot == n && steps == n && seen == tree.leaves.size(), "a stackless walk from node 0 sees every node and the leaves in depth-first order");
    bool padding = true;
    for (int k = 0; k < 8; k++)
        padding = padding && word(dn.quads, n, k) == 0u;
    rule(padding, "the last two quadwords are zero");
    rule(dn.boxesMayBeNan == (tree.anyNan ? 1u : 0u), "boxesMayBeNan exactly when a bound is NaN");
    /* the fold's count runs over these words (wpt_fold_plan, wpt_scene_folded_links) */
    std::vector<uint32_t> lds(n);
    const uint32_t folded = countFoldedLinks(reinterpret_cast<const uint32_t*>(dn.quads.data()), n, lds.data());
    bool inTree = folded <= n;
    for (uint32_t i = 0; i < n; i++)
        inTree = inTree && (word(dn.quads, i, 7) >= NODE_CHILD ? lds[i] <= n : lds[i] == ~word(dn.quads, i, 7));
    rule(inTree, "every word of the LDS copy is a node, the null node or a leaf's word complemented");
}

static void checkTriangles(const Scene& s, const Tree& tree, const std::vector<uint32_t>& triNew, uint64_t seed, int asGiven)
{
    const uint32_t T = s.d.tri_count;
    auto rule = [&](bool ok, const char* what) { check(ok, what, seed, 0, asGiven); };
    std::vector<uint32_t> old(T, 0xffffffffu);
    bool perm = triNew.size() == T;
    for (uint32_t t = 0; t < T && perm; t++) {
        perm = triNew[t] < T && old[triNew[t]] == 0xffffffffu;
        if (perm)
            old[triNew[t]] = t;
    }
    rule(perm, "triNew is a permutation");
    if (!perm)
        return;
    bool order = true;
    if (asGiven) {
        for (uint32_t t = 0; t < T; t++)
            order = order && triNew[t] == t;
    } else {
        std::vector<char> referred(T, 0);
        uint32_t next = 0;
        for (uint32_t l : tree.leaves)
            if (s.nodes[l].kind == WPT_NODE_TRIANGLE && !referred[s.nodes[l].link]) {
                referred[s.nodes[l].link] = 1;
                order = order && triNew[s.nodes[l].link] == next++;
            }
        for (uint32_t t = 0; t < T; t++)
            if (!referred[t])
                order = order && triNew[t] == next++;
    }
    rule(order, asGiven ? "as given: the identity" : "first references along the leaves in increasing order, then the triangles without a leaf in their own");
    const std::vector<wpt_tri_geom> g = permuted(s.d.tri_geom, triNew);
    const std::vector<wpt_tri_attr> a = permuted(s.d.tri_attr, triNew);
    bool moved = g.size() == T && a.size() == T;
    for (uint32_t t = 0; t < T && moved; t++)
        moved = memcmp(&g[triNew[t]], &s.geom[t], sizeof(wpt_tri_geom)) == 0 && memcmp(&a[triNew[t]], &s.attr[t], sizeof(wpt_tri_attr)) == 0;
    rule(moved, "geometry and attribute records moved with their triangle");
    const std::vector<wpt_hotspot> h = remappedHotspots(&s.d, triNew);
    bool spots = h.size() == s.hotspots.size();
    for (size_t k = 0; k < h.size() && spots; k++) {
        wpt_hotspot want = s.hotspots[k];
        if (want.kind != WPT_HOTSPOT_SPHERE)
            want.prim = triNew[want.prim];
        spots = memcmp(&h[k], &want, sizeof(want)) == 0;
    }
    rule(spots, "triangle hot spots are remapped, sphere hot spots are not");
}

/* the wide form against the binary tree: expansion, bounds, references, creation order, and the walk's pending entries */
static void checkWide(const Scene& s, const Tree& tree, const std::vector<uint32_t>& triNew, bool expectOffered, uint64_t seed, int asGiven)
{
    auto rule = [&](bool ok, const char* what) { check(ok, what, seed, 0, asGiven); };
    uint32_t worst = 0;
    const std::vector<Quad> wide = wideNodes(&s.d, triNew, &worst);
    rule(wide.empty() != expectOffered, expectOffered ? "the wide form is offered" : "the wide form is not offered");
    if (wide.empty())
        return;
    const size_t wideCount = wide.size() / 8;
    struct Pending {
        uint32_t node; /* binary node of an entry */
        uint32_t wideIndex;
    };
    std::vector<Pending> stack;
    std::vector<uint32_t> leaves;
    size_t maxPending = 0, made = 1;
    bool bounds = true, refs = true, preorder = true;
    auto enter = [&](uint32_t w, uint32_t x) {
        /* the entries of the wide node of binary node x: its children, an inner child standing aside for its own two */
        std::vector<uint32_t> e;
        if (s.nodes[x].kind == WPT_NODE_INNER) {
            for (uint32_t c : { x + 1, s.nodes[x].link }) {
                if (s.nodes[c].kind == WPT_NODE_INNER) {
                    e.push_back(c + 1);
                    e.push_back(s.nodes[c].link);
                } else {
                    e.push_back(c);
                }
            }
        } else {
            e.push_back(x);
        }
        /* a wide node's 32 words: rows of four, lo.x lo.y lo.z hi.x hi.y hi.z, the references, one spare */
        auto at = [&](size_t row, size_t k) { return wordOf(wide, w, 32, 4 * row + k); };
        for (size_t k = 0; k < 4; k++) {
            const uint32_t ref = at(6, k);
            if (k >= e.size()) {
                refs = refs && ref == WIDE_NONE;
                continue;
            }
            const wpt_bvh_node& nd = s.nodes[e[k]];
            for (int a = 0; a < 3; a++)
                bounds = bounds && at(size_t(a), k) == bitsOf(nd.lo[a]) && at(size_t(3 + a), k) == bitsOf(nd.hi[a]);
            if (nd.kind == WPT_NODE_INNER && e[k] != x)
                refs = refs && ref >= NODE_CHILD && ref != WIDE_NONE && (ref & NODE_INDEX_MASK) < wideCount;
            else if (nd.kind == WPT_NODE_TRIANGLE)
                refs = refs && ref == triNew[nd.link];
            else if (nd.kind == WPT_NODE_SPHERE)
                refs = refs && ref == (PRIM_SPHERE | nd.link);
            else
                refs = refs && ref == WIDE_NONE;
        }
        for (size_t k = e.size(); k-- > 0;) {
            const Pending p = { e[k], at(6, k) };
            stack.push_back(p);
        }
    };
    enter(0, 0);
    while (!stack.empty() && refs) {
        const Pending p = stack.back();
        stack.pop_back();
        maxPending = std::max(maxPending, stack.size());
        const wpt_bvh_node& nd = s.nodes[p.node];
        if (nd.kind == WPT_NODE_INNER && p.node != 0) {
            preorder = preorder && (p.wideIndex & NODE_INDEX_MASK) == made; /* a wide node's first inner entry follows it */
            made++;
            enter(p.wideIndex & NODE_INDEX_MASK, p.node);
        } else if (nd.kind != WPT_NODE_EMPTY) {
            leaves.push_back(p.node);
        }
    }
    rule(refs, "every entry refers to its binary node's wide node, triangle or sphere");
    rule(bounds, "every entry's bounds are its binary node's");
    rule(preorder && made == wideCount, "wide nodes are made depth-first, one per inner entry");
    rule(leaves == tree.leaves, "expanding the wide tree depth-first gives the binary tree's leaves");
    rule(worst == maxPending && worst <= WIDE_STACK, "the stack's worst case is what a walk that enters everything keeps pending");
}

/* A tree whose wide walk keeps `pending` entries waiting.  A wide node with four entries whose first is inner leaves three
 * waiting while the walk is below it, so a chain of D such wide nodes, the last one's four entries all leaves, keeps 3 D
 * waiting: WIDE_STACK = 96 = 3 * 32 is a chain of 32.  One more -- 97 -- is the same chain with the last wide node's first
 * entry inner once more, over two leaves: that wide node has two entries and keeps one waiting.  So: pending = 3 D + r with
 * r = 0 (ends in four leaves) or r = 1 (ends in a pair below four entries).  Each link of the chain is the binary nodes
 * x (inner), c0 (inner), [entry 0 = the next link], leaf, c1 (inner), leaf, leaf.  All boxes are equal, which nests them. */
static Scene chainScene(uint32_t pending)
{
    Scene s = makeScene(1, 4);
    s.nodes.clear();
    const uint32_t D = pending / 3, r = pending % 3;
    wpt_bvh_node inner, leaf;
    memset(&inner, 0, sizeof(inner));
    for (int a = 0; a < 3; a++)
        inner.hi[a] = 1.0f;
    leaf = inner;
    inner.kind = WPT_NODE_INNER;
    leaf.kind = WPT_NODE_TRIANGLE;
    std::vector<uint32_t> open; /* x, c0 and c1 of every link, to be closed once the chain below them is laid down */
    for (uint32_t k = 0; k < D; k++) {
        open.push_back(uint32_t(s.nodes.size()));
        s.nodes.push_back(inner); /* x */
        s.nodes.push_back(inner); /* c0; its first child is the next link, or the chain's end */
    }
    if (r == 1) { /* a pair */
        s.nodes.push_back(inner);
        s.nodes.push_back(leaf);
        s.nodes.back().link = 1;
        s.nodes[s.nodes.size() - 2].link = uint32_t(s.nodes.size());
        s.nodes.push_back(leaf);
    } else {
        s.nodes.push_back(leaf);
    }
    while (!open.empty()) {
        const uint32_t x = open.back();
        open.pop_back();
        s.nodes[x + 1].link = uint32_t(s.nodes.size()); /* c0's second child */
        s.nodes.push_back(leaf);
        s.nodes.back().link = 2;
        s.nodes[x].link = uint32_t(s.nodes.size()); /* c1 */
        s.nodes.push_back(inner);
        s.nodes.back().link = uint32_t(s.nodes.size()) + 1;
        s.nodes.push_back(leaf);
        s.nodes.push_back(leaf);
        s.nodes.back().link = 3;
    }
    s.point();
    return s;
}

static void checkTexels(const Scene& s, uint64_t seed)
{
    size_t count = 0, sum = 0;
    const std::vector<wpt_texture> dev = texelOffsets(&s.d, &count);
    bool ok = dev.size() == s.textures.size();
    for (size_t k = 0; k < dev.size() && ok; k++) {
        wpt_texture want = s.textures[k];
        if (want.type == WPT_TEX_IMAGE) {
            want.texel_offset = sum;
            sum += size_t(want.width) * want.height;
        }
        ok = memcmp(&dev[k], &want, sizeof(want)) == 0;
    }
    check(ok && count == sum, "texel offsets: the running sum of width x height over the images, other records untouched", seed, 0, 0);
}

static void checkRgl(const Scene& s, uint64_t seed)
{
    auto rule = [&](bool ok, const char* what) { check(ok, what, seed, 0, 0); };
    const RglPool r = rglPool(&s.d);
    rule(r.pool.size() >= s.rglData.size() && memcmp(r.pool.data(), s.rglData.data(), s.rglData.size() * sizeof(float)) == 0, "the caller's pool is a prefix of the result");
    rule(r.rgbl.size() == s.brdfs.size(), "one table offset per measured BRDF");
    if (r.rgbl.size() != s.brdfs.size())
        return;
    int tables = 0;
    for (size_t i = 0; i < s.brdfs.size(); i++) {
        const wpt_rgl_brdf& b = s.brdfs[i];
        if (b.rgb.size_x != b.luminance.size_x) {
            rule(r.rgbl[i] == WPT_RGL_NONE, "a BRDF whose warps do not share their grids gets no table");
            continue;
        }
        tables++;
        const size_t at = r.rgbl[i], size = size_t(b.rgb.size_x) * b.rgb.size_y;
        const size_t records = size_t(b.luminance.param_size[0]) * b.luminance.param_size[1] * size;
        rule(r.rgbl[i] != WPT_RGL_NONE && at % 4 == 0 && at >= s.rglData.size() && at + 4 * records <= r.pool.size(), "an interleaved table starts on a multiple of four floats behind the caller's pool");
        if (r.rgbl[i] == WPT_RGL_NONE || at + 4 * records > r.pool.size())
            continue;
        bool values = true;
        for (uint32_t i0 = 0; i0 < b.luminance.param_size[0]; i0++)
            for (uint32_t i1 = 0; i1 < b.luminance.param_size[1]; i1++)
                for (size_t e = 0; e < size; e++) {
                    const size_t lumSlice = size_t(i0) * b.luminance.param_stride[0] + size_t(i1) * b.luminance.param_stride[1];
                    const float* rec = &r.pool[at + 4 * (lumSlice * size + e)];
                    for (uint32_t c = 0; c < 3; c++) {
                        const size_t slice = size_t(i0) * b.rgb.param_stride[0] + size_t(i1) * b.rgb.param_stride[1] + size_t(c) * b.rgb.param_stride[2];
                        values = values && bitsOf(rec[c]) == bitsOf(s.rglData[b.rgb.data + slice * size + e]);
                    }
                    values = values && bitsOf(rec[3]) == bitsOf(s.rglData[b.luminance.data + lumSlice * size + e]);
                }
        rule(values, "a record holds r, g, b and luminance of its grid point");
    }
    rule(tables == 1, "one of the two descriptors can be interleaved");
}

static std::vector<float> makeImportance(uint64_t seed, size_t bins)
{
    Rng rng(seed ^ 0xe17a1465ull);
    std::vector<float> imp(bins);
    for (float& v : imp) { /* ties and a few bright bins */
        const bool tie = rng.below(8) == 0, bright = rng.below(16) == 0;
        v = tie ? 0.25f : rng.unit() * 4.0f + (bright ? 100.0f : 0.0f);
    }
    return imp;
}

static void checkEnv(uint64_t seed, size_t bins)
{
    auto rule = [&](bool ok, const char* what) { check(ok, what, seed, 0, 0); };
    const std::vector<float> imp = makeImportance(seed, bins);
    const EnvTables t = envTablesFromImportance(imp.data(), bins);
    rule(t.M.size() == bins && t.Ms.size() == bins && t.Mcs.size() == bins, "three tables of one entry per bin");
    if (t.M.size() != bins || t.Ms.size() != bins || t.Mcs.size() != bins)
        return;
    float total = 0.0f;
    for (size_t i = 0; i < bins; i++)
        total += imp[i];
    bool normalised = true, perm = true, sorted = true, sums = true;
    std::vector<char> seen(bins, 0);
    float sum = 0.0f;
    for (size_t i = 0; i < bins; i++) {
        normalised = normalised && bitsOf(t.M[i]) == bitsOf(imp[i] / total);
        perm = perm && t.Ms[i] >= 0 && size_t(t.Ms[i]) < bins && !seen[size_t(t.Ms[i])];
        if (!perm)
            break;
        seen[size_t(t.Ms[i])] = 1;
        sorted = sorted && (i == 0 || t.M[size_t(t.Ms[i - 1])] >= t.M[size_t(t.Ms[i])]);
        sum += t.M[size_t(t.Ms[i])];
        sums = sums && bitsOf(t.Mcs[i]) == bitsOf(sum);
    }
    rule(normalised, "M is the importance over its sequential float sum");
    rule(perm, "Ms is a permutation");
    rule(sorted, "M[Ms[i]] never increases");
    rule(sums, "Mcs is the float running sum in that order");
    const std::vector<int32_t> lut = envStartTable(t.Mcs.data(), bins);
    rule(lut.size() == size_t(ENV_LUT_SIZE) + 1, "a monotone Mcs has a start table");
    if (lut.size() == size_t(ENV_LUT_SIZE) + 1) {
        bool first = lut[ENV_LUT_SIZE] == int32_t(bins - 1);
        for (uint32_t k = 0; k < ENV_LUT_SIZE && first; k++) {
            const float at = float(k) / 65536.0f;
            const size_t i = size_t(lut[k]);
            first = lut[k] >= 0 && i < bins && (i == 0 || t.Mcs[i - 1] < at) && (t.Mcs[i] >= at || i == bins - 1);
        }
        rule(first, "lut[k] is the first bin with Mcs >= k / 65536, clamped");
    }
    if (bins >= 3) {
        std::vector<float> dented = t.Mcs;
        dented[bins / 2] = dented[bins / 2 - 1] * 0.5f;
        rule(dented[bins / 2 - 1] > 0.0f && envStartTable(dented.data(), bins).empty(), "no start table for a non-monotone Mcs");
    }
}

/* ---- validate, then the layout, on damaged input ---- */

static uint32_t damagedWord(Rng& rng, uint32_t around)
{
    switch (rng.below(6)) {
    case 0: return uint32_t(rng.next());
    case 1: return 0xffffffffu - rng.below(3);
    case 2: return around + rng.below(3) - 1;
    case 3: return 0x7fffffffu + rng.below(3);
    default: return rng.below(around + 2);
    }
}

static void damage(Rng& rng, Scene& s)
{
    const wpt_scene_desc& d = s.d;
    for (uint32_t hits = 1 + rng.below(3); hits > 0; hits--) {
        switch (rng.below(14)) {
        case 0: s.nodes[rng.below(d.node_count)].link = damagedWord(rng, d.node_count); break;
        case 1: s.nodes[rng.below(d.node_count)].kind = rng.below(5); break;
        case 2: {
            /* two nodes trade places: links that are in range and describe another tree, or none */
            const uint32_t a = rng.below(d.node_count), b = rng.below(d.node_count);
            std::swap(s.nodes[a], s.nodes[b]);
            break;
        }
        case 3: {
            wpt_tri_geom& g = s.geom[rng.below(d.tri_count)];
            (rng.below(2) ? g.instance : g.material) = damagedWord(rng, 3);
            if (rng.below(3) == 0)
                g.flags = rng.below(16);
            break;
        }
        case 4: {
            wpt_hotspot& h = s.hotspots[rng.below(d.hotspot_count)];
            const uint32_t which = rng.below(3);
            if (which == 0)
                h.prim = damagedWord(rng, d.tri_count);
            else if (which == 1)
                h.kind = rng.below(3);
            else
                h.animation = int32_t(damagedWord(rng, d.animation_count));
            break;
        }
        case 5: {
            wpt_animation& a = s.animations[rng.below(d.animation_count)];
            (rng.below(2) ? a.first_keyframe : a.keyframe_count) = damagedWord(rng, d.keyframe_count);
            break;
        }
        case 6:
        case 7:
        case 8: {
            /* any word of a measured BRDF's five warps but the four floats at a warp's end */
            wpt_rgl_brdf& b = s.brdfs[rng.below(d.rgl_count)];
            wpt_rgl_warp* warps[5] = { &b.ndf, &b.sigma, &b.vndf, &b.luminance, &b.rgb };
            uint32_t* words = reinterpret_cast<uint32_t*>(warps[rng.below(5)]);
            const uint32_t k = rng.below(15);
            words[k] = k < 12 ? damagedWord(rng, words[k]) : damagedWord(rng, uint32_t(d.rgl_data_count));
            break;
        }
        case 9: {
            wpt_texture& t = s.textures[rng.below(d.texture_count)];
            const uint32_t which = rng.below(7);
            if (which == 0)
                t.type = rng.below(5);
            else if (which == 1)
                t.width = damagedWord(rng, t.width);
            else if (which == 2)
                t.height = damagedWord(rng, t.height);
            else if (which == 3)
                t.comps = rng.below(6);
            else if (which == 4)
                t.texel_type = rng.below(4);
            else if (which == 5)
                t.child = int32_t(damagedWord(rng, d.texture_count));
            else
                t.texel_offset = rng.below(2) ? damagedWord(rng, uint32_t(d.texel_bytes)) : rng.next();
            break;
        }
        case 10: {
            wpt_material& m = s.materials[rng.below(d.material_count)];
            const uint32_t which = rng.below(3);
            if (which == 0)
                m.type = rng.below(11);
            else if (which == 1)
                m.tex[rng.below(5)] = int32_t(damagedWord(rng, d.texture_count));
            else
                m.normal_tex = int32_t(damagedWord(rng, d.texture_count));
            break;
        }
        case 11: {
            wpt_sphere& sp = s.spheres[rng.below(d.sphere_count)];
            if (rng.below(2))
                sp.material = damagedWord(rng, d.material_count);
            else
                sp.animation = int32_t(damagedWord(rng, d.animation_count));
            break;
        }
        case 12: {
            wpt_instance& in = s.instances[rng.below(d.instance_count)];
            if (rng.below(2))
                in.animation = int32_t(damagedWord(rng, d.animation_count));
            else
                in.flags = rng.below(16);
            break;
        }
        default: {
            const uint32_t which = rng.below(3);
            if (which == 0)
                s.d.envmap.type = rng.below(4);
            else if (which == 1)
                s.d.envmap.tex = int32_t(damagedWord(rng, d.texture_count));
            else
                s.d.envmap.cube_tex[rng.below(6)] = int32_t(damagedWord(rng, d.texture_count));
            break;
        }
        }
    }
}

/* every layout function over a description validate() accepted; the sanitizers watch the indices */
static bool layOut(const Scene& s, uint32_t top, bool asGiven)
{
    const std::vector<uint32_t> triNew = triangleOrder(&s.d, asGiven);
    DeviceNodes dn;
    if (deviceNodes(&s.d, triNew, top, &dn).code != WPT_OK)
        return false;
    const uint32_t n = s.d.node_count;
    std::vector<uint32_t> lds(n);
    bool ok = countFoldedLinks(reinterpret_cast<const uint32_t*>(dn.quads.data()), n, lds.data()) <= n;
    uint32_t slot = 0, steps = 0;
    while (slot < n && steps <= n) { /* the walk ends */
        const uint32_t w = word(dn.quads, slot, 7);
        slot = w >= NODE_CHILD ? (w & NODE_INDEX_MASK) : word(dn.quads, slot, 6);
        steps++;
    }
    ok = ok && slot == n && steps == n;
    const std::vector<Quad> wide = wideNodes(&s.d, triNew);
    ok = ok && wide.size() % 8 == 0;
    ok = ok && permuted(s.d.tri_geom, triNew).size() == s.d.tri_count && permuted(s.d.tri_attr, triNew).size() == s.d.tri_count;
    ok = ok && remappedHotspots(&s.d, triNew).size() == s.d.hotspot_count;
    size_t texels = 0;
    ok = ok && texelOffsets(&s.d, &texels).size() == s.d.texture_count;
    const RglPool r = rglPool(&s.d);
    return ok && r.pool.size() >= s.d.rgl_data_count && r.rgbl.size() == s.d.rgl_count;
}

static long fuzz(uint64_t scenes, uint32_t perScene, long* accepted)
{
    long damaged = 0;
    for (uint64_t seed = 1; seed <= scenes; seed++) {
        const Scene base = makeScene(0xd0000 + seed, 1 + uint32_t(seed % 24));
        Rng rng(seed * 77 + 5);
        for (uint32_t k = 0; k < perScene; k++) {
            Scene s = base;
            s.point();
            damage(rng, s);
            damaged++;
            if (validate(&s.d).code != WPT_OK)
                continue;
            *accepted += 1;
            const uint32_t n = s.d.node_count, tops[9] = { 0, 1, 2, 3, 7, n - 1, n, n + 1, 65536 };
            const uint32_t top = tops[rng.below(9)];
            check(layOut(s, top, rng.below(2) != 0), "an accepted description has a layout whose walk ends", 0xd0000 + seed, 0, 0);
        }
    }
    return damaged;
}

static void checkNullArrays(uint64_t seed)
{
    const Scene base = makeScene(seed, 9);
    const char* names[7] = { "tri_geom", "tri_attr", "instances", "materials", "textures", "hotspots", "texels" };
    for (int k = 0; k < 7; k++) {
        wpt_scene_desc d = base.d;
        switch (k) {
        case 0: d.tri_geom = nullptr; break;
        case 1: d.tri_attr = nullptr; break;
        case 2: d.instances = nullptr; break;
        case 3: d.materials = nullptr; break;
        case 4: d.textures = nullptr; break;
        case 5: d.hotspots = nullptr; break;
        default: d.texels = nullptr; break;
        }
        const Status st = validate(&d);
        check(st.code == WPT_ERR_INVALID_ARGUMENT && st.message && strstr(st.message, names[k]) && strstr(st.message, "NULL"), "a NULL array with a count is refused by name", seed, 0, k);
    }
    /* ... and an array without a count may be NULL */
    wpt_scene_desc d = base.d;
    Scene noTriangles = base;
    for (wpt_bvh_node& nd : noTriangles.nodes)
        if (nd.kind == WPT_NODE_TRIANGLE)
            nd.kind = WPT_NODE_EMPTY;
    for (wpt_hotspot& h : noTriangles.hotspots) {
        h.kind = WPT_HOTSPOT_SPHERE;
        h.prim = 0;
    }
    d.nodes = noTriangles.nodes.data();
    d.hotspots = noTriangles.hotspots.data();
    d.tri_count = 0;
    d.tri_geom = nullptr;
    d.tri_attr = nullptr;
    const Status st = validate(&d);
    check(st.code == WPT_OK, "arrays without a count may be NULL", seed, 0, 0);
    if (st.code == WPT_OK) {
        Scene s = noTriangles;
        s.d = d;
        check(layOut(s, 0, false), "a scene without triangles has a layout", seed, 0, 0);
    }
}

/* ---- digests ---- */

static uint64_t fnv(const void* data, size_t bytes)
{
    const uint8_t* p = static_cast<const uint8_t*>(data);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; i++)
        h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

template<typename T> static void digest(const char* name, uint64_t seed, uint32_t top, int asGiven, const std::vector<T>& v, bool none = false)
{
    if (none)
        printf("seed %" PRIu64 " top %u %s %s none\n", seed, top, asGiven ? "given" : "leaves", name);
    else
        printf("seed %" PRIu64 " top %u %s %s %016" PRIx64 "\n", seed, top, asGiven ? "given" : "leaves", name, fnv(v.data(), v.size() * sizeof(T)));
}

static int digests()
{
    const uint32_t sizes[6] = { 1, 5, 300, 2500, 4000, 50000 }; /* the last tree has more nodes than the default in front */
    for (uint64_t seed = 1; seed <= 6; seed++) {
        const Scene s = makeScene(0xa000 + seed, sizes[seed - 1]);
        if (validate(&s.d).code != WPT_OK)
            return 1;
        for (uint32_t top : { 0u, 7u, 65536u })
            for (int asGiven = 0; asGiven < 2; asGiven++) {
                const std::vector<uint32_t> triNew = triangleOrder(&s.d, asGiven != 0);
                DeviceNodes dn;
                if (deviceNodes(&s.d, triNew, top, &dn).code != WPT_OK)
                    return 1;
                digest("nodes", seed, top, asGiven, dn.quads);
                const std::vector<Quad> wide = wideNodes(&s.d, triNew);
                digest("wide", seed, top, asGiven, wide, wide.empty());
                digest("geometry", seed, top, asGiven, permuted(s.d.tri_geom, triNew));
                digest("attributes", seed, top, asGiven, permuted(s.d.tri_attr, triNew));
                digest("hotspots", seed, top, asGiven, remappedHotspots(&s.d, triNew));
                size_t texels = 0;
                digest("textures", seed, top, asGiven, texelOffsets(&s.d, &texels));
                const RglPool r = rglPool(&s.d);
                digest("rgl_pool", seed, top, asGiven, r.pool);
                digest("rgbl", seed, top, asGiven, r.rgbl);
                const size_t bins = 64 * 64;
                const std::vector<float> imp = makeImportance(seed, bins);
                const EnvTables t = envTablesFromImportance(imp.data(), bins);
                digest("env_M", seed, top, asGiven, t.M);
                digest("env_Ms", seed, top, asGiven, t.Ms);
                digest("env_Mcs", seed, top, asGiven, t.Mcs);
                const std::vector<int32_t> lut = envStartTable(t.Mcs.data(), bins);
                digest("env_lut", seed, top, asGiven, lut, lut.empty());
            }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "--digests")
        return digests();
    long scenes = 0, offered = 0;
    for (uint64_t seed = 1; seed <= 40; seed++) {
        const uint32_t T = seed <= 8 ? uint32_t(seed) : seed % 5 == 0 ? 1500 + uint32_t(seed) * 70 : 10 + uint32_t(seed * seed) % 400;
        const Scene s = makeScene(seed, T);
        const Status st = validate(&s.d);
        check(st.code == WPT_OK, "a made description is valid", seed, 0, 0);
        if (st.code != WPT_OK)
            continue;
        scenes++;
        const Tree tree = readTree(s);
        const uint32_t n = s.d.node_count, tops[9] = { 0, 1, 2, 3, 7, n - 1, n, n + 1, 65536 };
        for (int asGiven = 0; asGiven < 2; asGiven++) {
            const std::vector<uint32_t> triNew = triangleOrder(&s.d, asGiven != 0);
            checkTriangles(s, tree, triNew, seed, asGiven);
            for (uint32_t top : tops)
                checkNodes(s, tree, triNew, top, seed, asGiven);
            checkWide(s, tree, triNew, true, seed, asGiven);
            offered++;
        }
        checkTexels(s, seed);
        checkRgl(s, seed);
        /* the three reasons not to offer the wide form, and a NaN for boxesMayBeNan */
        const std::vector<uint32_t> triNew = triangleOrder(&s.d, false);
        uint32_t innerNode = 0xffffffffu;
        for (uint32_t i = 0; i < n && innerNode == 0xffffffffu; i++)
            if (s.nodes[i].kind == WPT_NODE_INNER)
                innerNode = i;
        for (int form = 0; form < 3; form++) {
            Scene bad = s;
            bad.point();
            Rng rng(seed + 1000);
            wpt_bvh_node& nd = bad.nodes[rng.below(n)];
            if (form == 0)
                nd.lo[rng.below(3)] = std::numeric_limits<float>::quiet_NaN();
            else if (form == 1)
                nd.hi[rng.below(3)] = std::numeric_limits<float>::infinity();
            else if (innerNode != 0xffffffffu) {
                const int a = int(rng.below(3));
                wpt_bvh_node& child = bad.nodes[rng.below(2) ? innerNode + 1 : s.nodes[innerNode].link];
                child.hi[a] = std::nextafter(bad.nodes[innerNode].hi[a], std::numeric_limits<float>::infinity()); /* outside by one ulp */
            } else {
                continue;
            }
            const Tree badTree = readTree(bad);
            checkWide(bad, badTree, triNew, false, seed, form);
            checkNodes(bad, badTree, triNew, 7, seed, 0);
        }
    }
    for (uint32_t pending : { 3u, 4u, WIDE_STACK, WIDE_STACK + 1 }) {
        const Scene s = chainScene(pending);
        const bool valid = validate(&s.d).code == WPT_OK;
        check(valid, "the chain is a valid tree", pending, 0, 0);
        if (!valid)
            continue;
        uint32_t worst = 0;
        const std::vector<uint32_t> triNew = triangleOrder(&s.d, false);
        (void)wideNodes(&s.d, triNew, &worst);
        check(worst == pending, "a chain built for a worst case has it", pending, 0, 0);
        checkWide(s, readTree(s), triNew, pending <= WIDE_STACK, pending, 0);
        checkNodes(s, readTree(s), triNew, 7, pending, 0);
    }
    for (uint64_t seed = 1; seed <= 6; seed++)
        checkEnv(seed, seed == 1 ? 1 : seed == 2 ? 3 : size_t(1) << (2 * seed));
    const int want[4][2] = { { 1, 0 }, { 12, -1 }, { 16, 4 }, { 512, 9 } };
    for (const int* w : want)
        check(envLog2(w[0]) == w[1], "envLog2", uint64_t(w[0]), 0, 0);
    checkNullArrays(3);
    long accepted = 0;
    const long damaged = fuzz(2000, 60, &accepted);
    check(accepted * 20 >= damaged, "validate still accepts one damaged description in twenty: the layout is exercised", 0, 0, 0);
    printf("%ld descriptions, %ld checks, %ld wide forms; %ld damaged descriptions, %ld of them valid and laid out; %ld failures\n", scenes, checksRun, offered,
            damaged, accepted, failures);
    return failures ? 1 : 0;
}
