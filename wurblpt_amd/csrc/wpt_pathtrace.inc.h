/*
 * wpt_pathtrace.inc.h -- the gfx950 path-tracing kernel (template; one translation unit per
 * instantiation, wpt_k_*.hip, so that the variants compile in parallel).
 *
 * Shape of the kernel, MI355X first:
 *
 *  - One lane owns one pixel and walks that pixel's whole sample sequence, because the
 *    reference seeds ONE Prng per pixel and consumes it serially over all samples
 *    (wurblpt.hpp:342-366).  Pixels are the only parallel axis; a wave is an 8x8 pixel tile.
 *
 *  - Every lane is a small state machine (NEW ray -> NODE steps <-> LEAF tests -> SHADE or
 *    NEE-END -> ...).  The 64 lanes of a wave are in different states at any time, so the wave
 *    runs its own scheduler: each round it counts the lanes per state with ballots and runs
 *    either the traversal loop (left as soon as too few lanes remain in it) or one long round
 *    that serves the SHADE, NEE-END and NEW lanes together.  Lanes in other states simply wait.
 *    Each lane still executes its own operations in the reference's order, so results do not
 *    change; only SIMD utilisation does (v0 without the scheduler: 18 % active lanes).
 *
 *  - Registers hold the ray and the walk (origin, direction, reciprocals, shear, node, bound, best
 *    candidate: 24 words).  The rest of the path's state (32 words: generator, accumulators,
 *    attenuations, the continuation behind a next-event ray) lives in LDS, eight 16-byte slots per
 *    lane (wpt_blocks.h): 32 KiB per 256-thread workgroup, so four workgroups per CU still fit, and
 *    the long round no longer spills the waiting lanes' words to scratch memory.
 *
 *  - BVH traversal is stackless.  The reference walks its depth-first node array with a stack,
 *    left child first (bvh.hpp:277-311); the node a pop returns to is always the first node behind
 *    the current subtree in depth-first order, so each device node carries that node's index
 *    ("skip") and an inner node the index of its first child: box hit & inner -> first child;
 *    leaf -> test it, then skip; otherwise -> skip.  Same visiting order, no stack, and the nodes
 *    may be STORED in any order (wpt_scene_layout.h lays the top of a large tree out level by level).
 *
 *  - Small scenes (nodes + triangle positions up to 20 KiB, e.g. the Cornell box: 4 KiB) are
 *    copied into LDS once per workgroup and traversed from there; larger scenes are fetched
 *    from HBM/L2 as two dwordx4 per node and three per triangle.
 *
 *  - The Cornell class's product kernel has a large form, wpt_pathtrace_large: one workgroup of 1024 lanes per compute unit,
 *    whose LDS holds the scene once instead of four times and, in the room that frees, the node array once per sign octant
 *    of a ray's direction, so that a box test sorts nothing (wpt_pathtrace_body.inc.h, ldsStep; wpt_kernel_table.h,
 *    selectLargeForm).
 *
 *  - Shading data (96 B per triangle) is read once per ray, after traversal.
 *  - No MFMA: there is no dense contraction anywhere on this path.
 */
#ifndef WPT_PATHTRACE_INC_H
#define WPT_PATHTRACE_INC_H

#include <hip/hip_runtime.h>

#include "../../include/wurblpt_hip.h"
#include "wpt_blocks.h"
#include "wpt_lds_places.h"

namespace wptk {

using namespace wptd;

constexpr int WG = 256; /* threads per workgroup: 4 waves, one per SIMD */
/* the large form of the two rotated kernels with the scene in LDS (wpt_pathtrace_large below): one workgroup of 16 waves per
 * compute unit, the same 1024 resident lanes as four workgroups of WG, but one copy of the scene in the unit's LDS instead of
 * four -- the room that the ordered box copies take (wpt_scene_layout.h, orderedBoxCopies) */
constexpr int WG_LARGE = 1024;
constexpr uint32_t LDS_BYTES_PER_CU = 160 * 1024; /* what one workgroup may declare */
constexpr uint32_t COLD_AT_LARGE = 32 * 1024;       /* the large form's cold path words: the last 128 KiB (wpt_pathtrace_body.inc.h) */
/* (ORDERED_COPIES, orderedPlaces and hitDataPlaces -- the node arrays of the ordered form, one per sign octant, where they lie, and
 * what of a hit's data follows them: wpt_lds_places.h) */
/* measurements: a library built with -DWPT_LARGE_PLAIN_STEP has the large form with the one node array and the sorting box
 * test of the small one, which tells what the workgroup's size costs or gains on its own */
#ifdef WPT_LARGE_PLAIN_STEP
constexpr bool LARGE_ORDERED = false;
#else
constexpr bool LARGE_ORDERED = true;
#endif
/* device node, word 7: a triangle index (< 2^31), PRIM_SPHERE | sphere index (< 2^30), or NODE_CHILD | index of the
 * first child (an empty node: NODE_CHILD | its own skip link, so that entering it is the same as skipping it) */
constexpr uint32_t NODE_CHILD = 0xc0000000u;
constexpr uint32_t NODE_INDEX_MASK = 0x3fffffffu;
/* dynamic LDS of a workgroup: the tables of expf / powf (wpt_math.h, 512 B), the paths' cold words (32 KiB), then the
 * scene if it is small */
constexpr uint32_t TABLE_BYTES = WPT_MATH_TABLE_WORDS * 8;
constexpr uint32_t COLD_BYTES = TABLE_BYTES + SLOT_COUNT * WG * 16;
/* with the scene behind them three workgroups still fit into a CU's 160 KiB */
constexpr uint32_t LDS_SCENE_MAX_BYTES = 20 * 1024;
/* a quarter of a compute unit's 160 KiB: what a workgroup may use where four of them are to share the unit (the material
 * records join the scene in LDS where they still fit into it) */
constexpr uint32_t LDS_BYTES_PER_WORKGROUP_AT_FOUR = 160 * 1024 / 4;
/* KernelArgs::materialsInLds is a word of bits for the kernels with the scene in LDS */
constexpr uint32_t LDS_MATERIALS = 1u; /* the material records are in LDS too */
constexpr uint32_t LDS_FOLD = 2u;      /* the LDS copy of the tree folds first children that repeat their parent's box (wpt_fold.h) */
constexpr uint32_t LDS_LEAF_LINKS = 4u; /* ROTATED kernels: a leaf's skip links are those in its triangle's corner records (every triangle has one leaf) */
/* the large form: the parts of a hit's data that follow the node copies in LDS (wpt_lds_places.h), HIT_DATA_* << LDS_HIT_DATA_SHIFT
 * -- the launcher picks the instantiation by them -- with HIT_DATA_MATERIALS beside them where the kernel reads the material
 * records by LDS address (materialPlaces), and in the word's upper half the instances whose normal matrices HIT_DATA_NORMALS holds */
constexpr uint32_t LDS_HIT_DATA_SHIFT = 8, LDS_HIT_NORMALS_SHIFT = 16;
/* ROTATED kernels, the leaf word of the tree's copy in LDS (wpt_leaf_words.h; wpt_capi.hip asserts that they agree):
 * sign bit | the leaf's node index << LEAF_NODE_SHIFT | quadword offset of the triangle's first corner within a copy */
constexpr uint32_t LEAF_NODE_SHIFT = 16, LEAF_NODE_MAX = 0x7fffu, LEAF_CORNER_MASK = 0xffffu;
/* the material records are copied to LDS quadword by quadword and read there through a generic pointer */
static_assert(sizeof(wpt_material) % 16 == 0 && alignof(wpt_material) <= 16, "wpt_material must be a whole number of quadwords");
/* A batch of views (FEAT_VIEWS kernels): the launch's lane indices g in [0, viewCount * viewPixels) are view g / viewPixels,
 * pixel g % viewPixels of that view's frame; view v is rendered from cams[v] into frame + v * viewPixels * 3.  A pixel's
 * generator is seeded from its index in its own frame, so view v is the plain render of cams[v] bit for bit.
 * Sample streams: with `streams`, pixel p of view v is seeded from the 64-bit index p + streams[v] * viewPixels instead, and
 * everything else stays the plain render; stream 0 is the plain render, and streams of one frame never share an index. */
struct ViewsView {
    const wpt_camera* cams; /* viewCount cameras in device memory */
    uint32_t viewPixels;    /* width * height */
    uint32_t viewCount;
    const uint32_t* streams; /* viewCount stream numbers in device memory, or NULL: all 0 */
};
/* Adaptive sampling (FEAT_ADAPTIVE kernels): pixel p is rendered with n_p^2 samples, n_p = samplesSqrt[p], with the strata,
 * 1 / n_p and 1 / n_p^2 of the plain render at samplesSqrt = n_p, so that its value is that render's bit for bit; a pixel with
 * n_p = 0 is not rendered and nothing of it is written.  moments (or NULL): per pixel and channel, 1 / n_p^2 times the fp32 sum
 * over the samples, in their order, of S * S, where S is what the sample added to that channel of the accumulator.  M is
 * read-added-written in HBM at each sample's end (a lane owns its pixel: no atomics), S is kept in registers (PathLdsSum). */
struct AdaptiveView {
    const uint16_t* samplesSqrt; /* [height][width] in device memory */
    float* moments;              /* [height][width][3] in device memory, or NULL */
};
/* Pixels in slices (FEAT_SLICED kernels, pooled launches): every pixel is cut into `units` units of `rows` rows of strata, and
 * the pool hands out indices in [0, units * blockSize): index `at` is unit g = at / blockSize of the pixel behind slot
 * at % blockSize -- all first units in the frame's order, then all second units, and so on.  The work unit that ends the launch
 * is then 1 / units of a pixel.  A pixel's samples stay one sequence from one generator: the lane that ends unit g - 1 stores
 * the generator and the sum (carry, the two quadwords of a first pass) and sets bit g of the slot's word, "unit g is ready"; the
 * lane that draws unit g sets bit 16 + g, "unit g was drawn".  Each does so with one atomic OR and looks at what the other had
 * set before: the drawer runs the unit if it was ready and otherwise goes back to the pool, and the lane that finds its next
 * unit already drawn runs it itself, straight on.  Exactly one of the two runs the unit, and neither waits for the other.
 * The OR that says "ready" is a release at agent scope and the drawer's OR an acquire, so that the carry crosses the L2s of
 * the XCDs; that costs a write-back of the L2 on one side and an invalidation on the other, which is what a unit's start costs
 * (with acquire and release on both sides the frame of 64 pixels per lane and 64 spp took 1389 ms instead of 937; 817 unsliced). */
struct SlicesView {
    uint32_t* words;           /* per slot, zero at the launch: bit g = unit g is ready, bit 16 + g = unit g was drawn and declined */
    float4* carry;             /* per slot: prng slot, acc slot */
    unsigned long long* stats; /* [0] units taken over by the lane that drew them, [1] units their pixel's lane ran on with */
    uint32_t rows, units;      /* units <= SLICE_UNITS_MAX; (units - 1) * rows < samplesSqrt <= units * rows */
    uint32_t declineOdd;       /* tests: units of odd slots are never taken over (their pixel's lane runs them all) */
};
constexpr uint32_t SLICE_UNITS_MAX = 15;      /* unit bits per half of a slot's word: g = 1 .. units - 1 */
constexpr uint32_t SLICE_SLOT_BITS = 28;      /* a lane keeps slot | g << 28 in one register */
constexpr uint32_t SLICE_SLOT_MASK = (1u << SLICE_SLOT_BITS) - 1u;
struct KernelArgs {
    SceneView sv;
    wpt_camera cam;
    wpt_params par;
    uint32_t width, height, samplesSqrt;
    float invWidth, invHeight, invSamplesSqrt, invSamples; /* 1.0f / (float)..., divided on the host */
    uint32_t blockStart, blockSize;
    uint32_t tiled; /* 1: a wave covers an 8x8 pixel tile (block is whole rows, multiple of 8) */
    /* bands: with bandStride > 0 the launch covers the bands of bandPixels consecutive pixels
     * whose index is bandFirst, bandFirst + bandStride, ... -- one rank's interleaved share of the frame in one launch;
     * blockStart is 0 and blockSize the number of lanes (pixels behind the end of the frame stay idle) */
    uint32_t bandPixels, bandFirst, bandStride;
    uint32_t leaveEighths; /* scheduler: leave the NODE loop when fewer than this many eighths of the entering lanes remain */
    uint32_t heavyMin;     /* scheduler: lanes a long block needs before it runs */
    uint32_t leafBias;     /* scheduler: leaf tests run when waiting lanes * leafBias >= walking lanes * 8 */
    uint32_t waitBelow;    /* scheduler: a kind of material with fewer lanes than this in a long round stands back once (0 = never) */
    uint32_t fuse;         /* scheduler: 1 = one long round serves SHADE, NEE-END and NEW lanes together */
    uint32_t shadowWalksEnd; /* 1: the walk of a light ray towards the environment ends at its first accepted hit (not in counting launches) */
    float* frame;
    /* Pixel pool (or NULL): lanes whose pixel is finished take the next lane index of the launch from this counter, which
     * starts at the number of lanes launched.  A launch then is as many workgroups as the GPU holds at once, and a wave
     * keeps its 64 lanes at work until the launch runs out of pixels instead of until its slowest pixel ends. */
    uint32_t* pool;
    /* Two passes over a frame (or NULL / 0): the first renders rowStop rows of every pixel's strata, stores what the pixel
     * carries on (generator, sum, next stratum) and the time it took; the second takes the pixels in `order` (the tiles
     * that took longest first, wpt_k_order.hip: the pixels that end the launch are the short ones) and goes on where the
     * first stopped.  A pixel's samples stay one sequence from one generator, so the frame is the same bit for bit. */
    uint32_t rowStop;             /* rows of strata to render in this launch; samplesSqrt: to the end */
    float4* carry;                /* per pixel of the frame: prng slot, acc slot */
    uint32_t* cost;               /* per pixel of the frame: shader clock of the first pass */
    const uint32_t* order;        /* second pass: pixels in the order they are handed out */
    const uint32_t* orderCount;   /* second pass: entries of `order` */
    uint32_t cuCount; /* for the launchers: compute units of the device */
    uint32_t materialsInLds; /* scene in LDS: LDS_MATERIALS (the material records are there too) | LDS_FOLD */
    wpt_counters* counters;
    unsigned long long* schedStats; /* COUNT builds: 16 scheduler statistics, or NULL */
    union { /* (no launch has both: the kernels of either feature are instantiated without the other) */
        BinsView bins;   /* FEAT_TRANSIENT kernels: the transient film (frame may be NULL there); FEAT_TOF kernels: the sensor and
                          * its phase planes (wpt_blocks.h, accumulate; with several phases frame is NULL) */
        ViewsView views; /* FEAT_VIEWS kernels: the batch's cameras; frame holds viewCount full frames, blockSize is all their pixels */
        AdaptiveView adaptive; /* FEAT_ADAPTIVE kernels: the sample-count map and the moment film; samplesSqrt above is unused */
        SlicesView slices; /* FEAT_SLICED kernels: the units pixels are handed out in (read only where the launch has a pool) */
        /* the FEAT_ANIM kernels of one plain frame, which have no member above: the rolling shutter (wpt_shutter.h; zeros, as a
         * launch's arguments start: none).  Every other kernel renders without one. */
        wptshutter::Rows shutter;
    };
};
/* the adaptive member must not change the union's size or the layout of what follows it: the existing kernels' code objects
 * stay as they were */
static_assert(sizeof(AdaptiveView) <= sizeof(BinsView) && alignof(AdaptiveView) <= alignof(BinsView), "AdaptiveView must fit in BinsView's place");
static_assert(sizeof(SlicesView) <= sizeof(BinsView) && alignof(SlicesView) <= alignof(BinsView), "SlicesView must fit in BinsView's place");
static_assert(sizeof(ViewsView) <= sizeof(BinsView) && alignof(ViewsView) <= alignof(BinsView), "ViewsView must fit in BinsView's place");
static_assert(sizeof(wptshutter::Rows) <= sizeof(BinsView) && alignof(wptshutter::Rows) <= alignof(BinsView), "the shutter must fit in BinsView's place");
/* the kernels that read KernelArgs::shutter: moving scenes, one plain frame (FEAT_SLICED has no moving-scene kernel) */
constexpr bool hasShutter(uint32_t F)
{
    return (F & FEAT_ANIM) != 0 && (F & (FEAT_TRANSIENT | FEAT_TOF | FEAT_VIEWS | FEAT_ADAPTIVE | FEAT_SLICED)) == 0;
}

/* lane index of the launch -> pixel; false: no pixel behind this index */
WPT_D bool lanePixel(const KernelArgs& args, uint32_t gid, uint32_t& pixel)
{
    bool inBlock = gid < args.blockSize;
    if (args.tiled) {
        const uint32_t tilesPerRow = args.width >> 3;
        const uint32_t tile = gid >> 6, lane = gid & 63u;
        const uint32_t tx = tile % tilesPerRow;
        uint32_t ty = tile / tilesPerRow;
        if (args.bandStride) {
            /* tile rows of this launch -> tile rows of the frame (bands are whole groups of 8 rows here) */
            const uint32_t tileRowsPerBand = args.bandPixels / (args.width << 3);
            ty = (args.bandFirst + (ty / tileRowsPerBand) * args.bandStride) * tileRowsPerBand + ty % tileRowsPerBand;
        }
        pixel = args.blockStart + ((ty << 3) + (lane >> 3)) * args.width + (tx << 3) + (lane & 7u);
    } else if (args.bandStride) {
        pixel = (args.bandFirst + (gid / args.bandPixels) * args.bandStride) * args.bandPixels + gid % args.bandPixels;
    } else {
        pixel = args.blockStart + gid;
    }
    if (args.bandStride && pixel >= args.width * args.height)
        inBlock = false; /* the last band may be shorter */
    if (!inBlock)
        pixel = args.blockStart;
    return inBlock;
}

/* lane states, in scheduling priority order for ties */
enum { S_NODE = 0, S_LEAF = 1, S_SHADE = 2, S_NEEEND = 3, S_NEW = 4, S_DONE = 5, S_START = 6 /* within a long round: has a ray to start */ };

/* ---- the wide walk (WIDE kernels; scenes fetched from HBM) ----
 * The binary tree collapsed by one level at upload (wpt_capi_scene.hip, SceneView::wideNodes): a wide node holds the boxes of a
 * node's up to four grandchildren (a child that is a leaf stands for itself) in the order BVH::hit comes to them
 * (bvh.hpp:277-311), and one step tests all four from one 128-byte line.  A child whose box the ray passes through under the
 * bound of that moment waits for its turn with its entry distance -- the next one in registers, the others on a small stack --
 * and is admitted at its turn if that distance is still within the bound, which is AABB::mayHit (aabb.hpp:70-86) under the
 * bound of its turn as long as (a) no slab distance is NaN and (b) the bound has not grown in between.  The inner nodes
 * that disappear decide nothing of their own: a child's box lies within its parent's (checked at upload) and the slab
 * arithmetic is monotone, so a child that passes implies the parent the reference tested before it.  Where (a) or (b) fails
 * the lane walks the binary tree instead, which IS the reference's walk:
 *   (a) a slab distance is NaN only for 0 * inf or inf - inf: a ray with a zero, infinite or NaN direction component, or an
 *       origin that is not finite (the boxes are finite: checked at upload), takes the binary walk from its start;
 *   (b) a hit is accepted by one comparison and its distance stored by another (hitable_triangle.hpp:283-296), so the bound
 *       can GROW by an ulp at a hit (one ray in 200 000 on the Sponza-class scene, tests/test_wide_walk.py); a lane that
 *       sees that starts its ray again from the root in the binary walk.
 * Checked on the CPU leaf test for leaf test against BVH::hit (oracle/wpt_oracle.cpp::bvhTraverseWide) and on the GPU bit for
 * bit against the oracle.  The stack cannot overflow: wpt_scene_upload offers the wide form only for trees whose worst case
 * fits WIDE_STACK entries. */
constexpr uint32_t WIDE_STACK = 96;          /* pending children per lane (8 bytes each, scratch memory): the 10 M triangle scene's worst case is 66 */
constexpr uint32_t WIDE_NONE = 0xffffffffu;  /* no child (also: an empty entry of a wide node) */
constexpr int RAY_WALK_BINARY = 0x80;        /* in RayAux::k: this ray walks the binary tree although its slab distances are numbers (its bound has grown) */

/* LDSSCENE: node n's pair of exact link words (a 32-bit byte offset from the uniform base: one register of address per lane) */
WPT_D uint2 exactLinks(const SceneView& sv, uint32_t n)
{
    return *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(sv.spheres) + (n << 3));
}

template<uint32_t F, bool COUNT, bool LDSSCENE, int OCC, bool WIDE = false>
__global__ __launch_bounds__(WG, OCC) void wpt_pathtrace(const KernelArgs args)
{
    constexpr int WGS = WG;
    constexpr bool ORDERED = false;
    constexpr uint32_t HIT = 0;
#include "wpt_pathtrace_body.inc.h"
}

/* the large form: a product kernel with the scene in LDS and one workgroup of WG_LARGE lanes per compute unit */
template<uint32_t F, int OCC, bool ORDERED, uint32_t HIT>
__global__ __launch_bounds__(WG_LARGE, OCC) void wpt_pathtrace_large(const KernelArgs args)
{
    constexpr int WGS = WG_LARGE;
    constexpr bool COUNT = false, LDSSCENE = true, WIDE = false;
#include "wpt_pathtrace_body.inc.h"
}

/* Launch of a product kernel.  With a pixel pool in the arguments and more workgroups than the device holds at once, the
 * launch shrinks to the resident workgroups and the counter starts behind their lanes; otherwise the pool stays unused. */
template<class Kernel>
inline void launchMaybePooled(Kernel kernel, const KernelArgs& args, dim3 grid, size_t ldsBytes, hipStream_t stream, int lanes = WG)
{
    KernelArgs a = args;
    /* more dynamic LDS than a kernel may have without asking (the large form); a refusal shows as the launch's error */
    if (ldsBytes > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    if (a.pool) {
        int perCu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, lanes, ldsBytes) != hipSuccess)
            perCu = 0;
        const uint64_t resident = (uint64_t)(perCu < 0 ? 0 : perCu) * a.cuCount;
        if (resident == 0 || grid.x <= resident
                || hipMemsetD32Async((hipDeviceptr_t)a.pool, (int)(resident * lanes), 1, stream) != hipSuccess)
            a.pool = nullptr;
        else
            grid.x = (uint32_t)resident;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(lanes), ldsBytes, stream, a);
}

constexpr uint32_t FEAT_BASIC = FEAT_GGX | FEAT_GLASS;
constexpr uint32_t FEAT_ALL = FEAT_TEXTURES | FEAT_MODPHONG | FEAT_ENVMAP | FEAT_LENS | FEAT_TWOSIDED | FEAT_GGX | FEAT_GLASS | FEAT_SPHERES | FEAT_SPOT;

/* getGroundTruth (wpt_k_groundtruth.hip): array[k] is the device array of GroundTruth bit k or NULL */
struct GroundTruthArgs {
    SceneView scene;
    wpt_camera cam, camPrev, camNext;
    wpt_params par;
    float t0, tPrev, tNext;
    uint32_t width, height;
    void* array[WPT_GT_ARRAY_COUNT];
};
void launchGroundTruth(const GroundTruthArgs& args, hipStream_t stream);
/* test hook (wpt_selftest_hits): the ground truth kernel's walk and finishHit for n given rays (origin, direction, amin, amax) */
void launchSelftestHits(const SceneView& scene, int n, const float* rays8, float* out15, hipStream_t stream);

/* wpt_k_order.hip: from the first pass's times to the second pass's order of pixels, longest first.  `work` is
 * 3 * ORDER_BUCKETS + 1 words of device memory; work[3 * ORDER_BUCKETS] receives the number of pixels in `order`. */
constexpr uint32_t ORDER_BUCKETS = 128;
void launchOrderBuild(const KernelArgs& args, uint32_t* order, uint32_t* work, hipStream_t stream);
/* One launcher per instantiation of wpt_pathtrace, each defined in its own translation unit (wpt_k_basic*.hip, wpt_k_full*.hip)
 * by one line of WPT_PATHTRACE_LAUNCHER; wpt_kernel_table.h lists them all.  sceneLdsBytes is the size of the scene copy behind
 * the cold path words in LDS, 0 for the kernels that fetch the scene from HBM.  OCC is the unit's own business: a launcher is
 * named by what the host chooses between. */
template<uint32_t F, bool COUNT, bool LDSSCENE, bool WIDE>
void launchPathtrace(const KernelArgs& args, dim3 grid, size_t sceneLdsBytes, hipStream_t stream);
#define WPT_PATHTRACE_LAUNCHER(F, COUNT, LDSSCENE, OCC, WIDE)                                                                  \
    template<> void launchPathtrace<(F), COUNT, LDSSCENE, WIDE>(const KernelArgs& args, dim3 grid, size_t sceneLdsBytes, hipStream_t stream) \
    {                                                                                                                          \
        launchMaybePooled(wpt_pathtrace<(F), COUNT, LDSSCENE, OCC, WIDE>, args, grid, COLD_BYTES + sceneLdsBytes, stream);     \
    }
/* The large form of the rotated kernels with the scene in LDS, FEAT_BASIC | FEAT_ROTATED and its sliced twin, each in a unit of
 * its own (wpt_k_basic_lds_rot_large.hip, wpt_k_basic_lds_rot_sliced_large.hip).  grid counts workgroups of WG_LARGE lanes;
 * sceneLdsBytes: the node array's copies, the corners' three rotations and the material records where they are in LDS. */
constexpr uint32_t COLD_BYTES_LARGE = TABLE_BYTES + SLOT_COUNT * WG_LARGE * 16;
static_assert(COLD_AT_LARGE + SLOT_COUNT * WG_LARGE * 16 == LDS_BYTES_PER_CU && TABLE_BYTES <= COLD_AT_LARGE, "the large form's cold words end the unit's LDS");
static_assert(LARGE_SCENE_ROOM_QUADS * 16 == COLD_AT_LARGE - TABLE_BYTES, "wpt_lds_places.h restates the room between the math tables and the cold words");
template<uint32_t F>
void launchPathtraceLarge(const KernelArgs& args, dim3 grid, size_t sceneLdsBytes, hipStream_t stream);
#define WPT_PATHTRACE_LARGE_LAUNCHER(F, OCC, ORDERED)                                                                          \
    template<> void launchPathtraceLarge<(F)>(const KernelArgs& args, dim3 grid, size_t sceneLdsBytes, hipStream_t stream)     \
    {                                                                                                                          \
        /* (the cold words lie at a fixed place behind the scene's room: the request is the whole unit's, whatever the scene's size) */   \
        if (COLD_BYTES_LARGE + sceneLdsBytes > LDS_BYTES_PER_CU)                                                               \
            return;                                                                                                            \
        /* one instantiation per set of parts of a hit's data in LDS that a launch may name (hitDataKernelParts) */            \
        /* ... and, for the two that have parts, one more that reads the material records by LDS address (materialPlaces) */   \
        /* ... and, for those two, one more that reads the launch's constants from a record in LDS (launchRecordFits) */        \
        const uint32_t hit = (args.materialsInLds >> LDS_HIT_DATA_SHIFT) & (HIT_DATA_ALL | HIT_DATA_MATERIALS | HIT_DATA_LAUNCH); \
        if (hit == (HIT_DATA_ALL | HIT_DATA_MATERIALS | HIT_DATA_LAUNCH))                                                      \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_ALL | HIT_DATA_MATERIALS | HIT_DATA_LAUNCH>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else if (hit == (HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS | HIT_DATA_MATERIALS | HIT_DATA_LAUNCH))                         \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS | HIT_DATA_MATERIALS | HIT_DATA_LAUNCH>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else if (hit == (HIT_DATA_ALL | HIT_DATA_MATERIALS))                                                                   \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_ALL | HIT_DATA_MATERIALS>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else if (hit == (HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS | HIT_DATA_MATERIALS))                                           \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS | HIT_DATA_MATERIALS>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else if (hit == HIT_DATA_ALL)                                                                                          \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_ALL>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else if (hit == (HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS))                                                                \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, HIT_DATA_RECORDS | HIT_DATA_HOTSPOTS>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE); \
        else                                                                                                                   \
            launchMaybePooled(wpt_pathtrace_large<(F), OCC, ORDERED, 0u>, args, grid, LDS_BYTES_PER_CU, stream, WG_LARGE);     \
    }
/* wpt_k_adaptive_cost.hip: args.cost[p] = n_p^2 for the block's pixels, the order's measure of an adaptive launch */
void launchAdaptiveCost(const KernelArgs& args, hipStream_t stream);

} /* namespace wptk */

#endif
