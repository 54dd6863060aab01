/*
 * wpt_pathtrace_body.inc.h -- the body of the path-tracing kernels, included into each of the two kernel templates of
 * wpt_pathtrace.inc.h (which says what the kernel is): as program text and not as a function, so that the kernel of WG lanes
 * compiles to the code it had before there was a second one.  The including kernel names, as template parameters or constants:
 * F, COUNT, LDSSCENE, WIDE; WGS, the lanes of its workgroup; ORDERED (the large form only): the tree lies in LDS once per sign
 * octant with the bounds of the negative axes mirrored, and a ray without RAY_MAY_NAN walks mirrored the same way, so that its
 * box test finds the six slab distances sorted (ldsStep); HIT (the large form only): the parts of a hit's data that lie in LDS
 * behind the node copies (wpt_lds_places.h).
 */
    static_assert(!ORDERED || ((F & FEAT_ROTATED) && LDSSCENE && WGS == WG_LARGE), "ordered box copies: the large form of the rotated kernels with the scene in LDS");
    static_assert(!WIDE || (!LDSSCENE && !COUNT), "the wide walk: product kernels that fetch the scene from HBM (counting launches walk like the reference)");
    static_assert(!LDSSCENE || !(F & FEAT_SPHERES), "the LDS copy of the tree tells leaves (complemented word) from inner nodes by the sign bit: triangle leaves only");
    static_assert(!((F & FEAT_VIEWS) && (F & FEAT_TRANSIENT)), "a batch of views has no transient film (they share KernelArgs' union)");
    static_assert(!((F & FEAT_ADAPTIVE) && (F & (FEAT_VIEWS | FEAT_TRANSIENT))), "adaptive sampling has no views and no transient film (they share KernelArgs' union)");
    static_assert(!((F & FEAT_ADAPTIVE) && COUNT), "adaptive sampling has no counting build");
    static_assert(!((F & FEAT_TOF) && ((F & (FEAT_VIEWS | FEAT_TRANSIENT | FEAT_ADAPTIVE)) || COUNT)), "the time-of-flight sensor: one view, no other film, no counting build");
    static_assert(!((F & FEAT_SLICED) && ((F & (FEAT_VIEWS | FEAT_TRANSIENT | FEAT_ADAPTIVE | FEAT_TOF)) || COUNT)), "pixels in slices: plain product launches (they share KernelArgs' union)");
    static_assert(!LDSSCENE || (!WIDE && !(F & FEAT_SPHERES)), "the kernels with the scene in LDS carry their link words in SceneView::wideNodes and ::spheres (wpt_device.h): they may read neither as what it is named");
    constexpr bool VIEWS = (F & FEAT_VIEWS) != 0;
    constexpr bool ADAPTIVE = (F & FEAT_ADAPTIVE) != 0;
    constexpr bool SLICED = (F & FEAT_SLICED) != 0;
    /* the corners in LDS three times, once per rotation of (x, y, z): a triangle test reads them in its ray's component order */
    constexpr bool ROTATED = (F & FEAT_ROTATED) != 0;
    static_assert(!ROTATED || (LDSSCENE && !(F & FEAT_ANIM)), "rotated copies of the corners: scenes at rest in LDS");
    /* node prefetch: for scenes in HBM (Sponza-class frame 3 % faster); not from LDS, where the fetch is short and the
     * registers that hold the node ahead lengthen every step (Cornell 4 % slower) */
    constexpr bool PREFETCH = !LDSSCENE && !WIDE;
    /* Node steps per look at the lane counts.  The look itself (two ballots, their counts, the leave and leaf decisions:
     * some twenty scalar instructions and two branches in every lane's way) costs a wave as much issue time as half a
     * node step.  From LDS a step is short, and taking up to three in a row before looking again gave 852 against 799
     * Msamples/s on the Cornell frame (2: 839, 4: 841, 6: 836, 8: 791: lanes that reach a leaf wait out the rest); from
     * HBM the steps are memory round trips and nothing is gained. */
    constexpr int STEPS = LDSSCENE ? 3 : 1;
    /* Lanes at the end of a light ray that the walk serves itself (0: they wait for the long round).  Kernels that fetch the scene
     * from HBM wait for memory, not for instruction issue: there a lane that walks on sooner is worth the extra run of the short
     * block (Sponza-class 152.7 -> 158.0 Msamples/s with 3 or 4 lanes, 157.3 / 156.8 with 8 / 12, 155.1 with 2; measured BRDFs in
     * the single kernel 106.1 -> 112.5; 10 M triangles 67.97 -> 68.09).  With the scene in LDS the frame is bound by the
     * instructions its waves issue and the same costs (Cornell 1055.6 against 1038.7 / 1049.1 / 1036.0 with 8 / 16 / 24). */
    constexpr int NEE_IN_WALK = LDSSCENE ? 0 : 4;
    /* ROTATED: a wave's issue priority by phase, set at the two wave-uniform points where the scheduler has picked (s_setprio is a
     * scalar instruction and does not look at the exec mask).  A wave in the walk issues short bursts between LDS round trips
     * and is ready for a few cycles at a time; a wave in the long round has long runs of independent arithmetic and loses
     * little when it yields.  Walk above long round: Cornell 1493.9 - 1497.2 against 1484.5 - 1486.7 Msamples/s; the reverse
     * 1465.1 - 1466.4; priority 1 for two of a workgroup's four waves throughout 1479.4 - 1480.5
     * (profiles/leaf_words_cornell.txt). */
    constexpr int PRIORITY_WALK = 2, PRIORITY_LONG = 0;
    /* [ math tables ][ cold path words: SLOT_COUNT x WG float4 ][ LDSSCENE: nodes, triangle positions (ROTATED: and their two
     * rotated copies), material records where they fit ] */
    extern __shared__ float4 lds[];
    /* The large form: [ math tables ][ the scene ][ cold path words at COLD_AT_LARGE, to the end of the unit's LDS ], the cold
     * words as four blocks of SLOT_COUNT x WG float4, one per 256 lanes.  So the scene lies within the 64 KiB that the offset
     * field of an LDS instruction reaches, and a lane's slots lie 4 KiB apart as in the small form: no slot and no node costs
     * an address instruction more than there. */
    constexpr bool LARGE = WGS == WG_LARGE;
    float4* const ldsCold = LARGE ? lds + COLD_AT_LARGE / 16 : lds + TABLE_BYTES / 16;
    float4* const ldsScene = LARGE ? lds + TABLE_BYTES / 16 : ldsCold + SLOT_COUNT * WGS;
#if defined(WPT_MATH_TABLES_IN_LDS) && defined(__HIP_DEVICE_COMPILE__)
    wptm::tables_to_lds(threadIdx.x);
#endif

    /* the kernel with the scene in LDS points its own copy of the scene view at the material records there; the others
     * read the launch arguments where they lie (a copy costs the all-features kernel 2 %) */
    SceneView svInLds = args.sv;
    const SceneView& sv = LDSSCENE ? static_cast<const SceneView&>(svInLds) : args.sv;
    const wpt_params& par = args.par;
    const uint32_t nodeCount = sv.nodeCount;
    uint32_t orderedBase = 0, orderedStride = 0; /* ORDERED: copy k >= 1 of the node array lies orderedBase + k * orderedStride quadwords behind copy 0 */
    LdsHitData<HIT> hitData = {}; /* LARGE: the corners and, behind the node copies, the parts HIT of a hit's data in LDS (wpt_device.h) */

    if (LDSSCENE) {
        /* nodes (2 x float4 each), the null node, then the triangle positions (3 x float4 each).  The LDS copy of a node has
         * the walk's own two link words, made on the host once per scene (the words in sv.wideNodes' place, wpt_device.h; wpt_fold.h, wpt_bypass.h): the skip link,
         * and in word 7 the node a ray that passes an inner node's box goes to as a plain index -- its first child, with
         * LDS_FOLD what lies behind the first children that repeat its box, and either led on past the nodes the scene's plan
         * leaves out of the walk -- or a leaf's word complemented (>= 2^31; ROTATED: the leaf word of wpt_leaf_words.h, >= 2^31
         * as well, in the sets these kernels are given); links clamped to nodeCount.  The null node (index
         * nodeCount: skip and child both nodeCount) is where every lane that does not walk stands, so that a step leaves it
         * where it is whatever its box test says. */
        const uint32_t n4 = 2 * nodeCount, t4 = 3 * sv.triCount;
        for (uint32_t i = threadIdx.x; i < n4; i += WGS) {
            float4 q = sv.nodes[i];
            if (i & 1) {
                const uint2 links = reinterpret_cast<const uint2*>(sv.wideNodes)[i >> 1];
                q.z = __uint_as_float(links.x);
                q.w = __uint_as_float(links.y);
            }
            ldsScene[i] = q;
        }
        if (threadIdx.x < 2)
            ldsScene[n4 + threadIdx.x] = threadIdx.x == 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)
                    : make_float4(0.0f, 0.0f, __uint_as_float(nodeCount), __uint_as_float(nodeCount));
        if (ROTATED) {
            /* the stored order (that of kz = 2) and the copies for rays whose largest direction component is x (kz = 0: y, z, x)
             * and y (kz = 1: z, x, y), records of the same shape behind the stored ones (rotatedCopyOffset).  The fourth words
             * of a triangle's three records are what a leaf pass needs beside the corners, made once per scene on the host
             * (wpt_leaf_words.h, behind the link words): its leaf's skip link under the launch's links, the exact one, and the
             * triangle's index.  (What finishHit reads in their place comes from the records in HBM, or with HIT from the hit records below.) */
            const uint32_t* const triSkip = reinterpret_cast<const uint32_t*>(sv.wideNodes) + n4 + 4;
            const uint32_t* const triExact = reinterpret_cast<const uint32_t*>(sv.spheres) + n4 + 4;
            for (uint32_t i = threadIdx.x; i < t4; i += WGS) {
                const float4 g = sv.triGeom[i];
                const uint32_t tri = i / 3u, corner = i - 3u * tri;
                const float w = __uint_as_float(corner == 0 ? triSkip[tri] : corner == 1 ? triExact[tri] : tri);
                ldsScene[n4 + 2 + i] = make_float4(g.x, g.y, g.z, w);
                ldsScene[n4 + 2 + t4 + i] = make_float4(g.y, g.z, g.x, w);
                ldsScene[n4 + 2 + 2 * t4 + i] = make_float4(g.z, g.x, g.y, w);
            }
        } else {
            for (uint32_t i = threadIdx.x; i < t4; i += WGS)
                ldsScene[n4 + 2 + i] = sv.triGeom[i];
        }
        const uint32_t c4 = ROTATED ? 3 * t4 : t4; /* quadwords of triangle positions in LDS */
        if (args.materialsInLds & LDS_MATERIALS) {
            /* the material record is what a hit's shading waits for first: fetched from LDS through a generic pointer */
            const uint32_t m4 = sv.materialCount * (uint32_t)(sizeof(wpt_material) / 16);
            const float4* from = reinterpret_cast<const float4*>(sv.materials);
            for (uint32_t i = threadIdx.x; i < m4; i += WGS)
                ldsScene[n4 + 2 + c4 + i] = from[i];
            svInLds.materials = reinterpret_cast<const wpt_material*>(ldsScene + n4 + 2 + c4);
        }
        if constexpr (ORDERED) {
            /* behind all that, copies 1 .. 7 of the node array (wpt_scene_layout.h, orderedBoxCopies: the launch carries the
             * eight in sv.rglData's place -- a kernel of the basic feature set has no measured BRDFs; copy 0 is the array
             * above), each with its null node and the same link words, copy k at orderedBase + k * orderedStride
             * (orderedPlaces: a node's eight records lie in eight different groups of banks) */
            const uint32_t m4 = (args.materialsInLds & LDS_MATERIALS) ? sv.materialCount * (uint32_t)(sizeof(wpt_material) / 16) : 0u;
            orderedPlaces(n4 + 2, c4 + m4, orderedBase, orderedStride);
            const float4* const copies = reinterpret_cast<const float4*>(sv.rglData);
            for (uint32_t i = n4 + 2 + threadIdx.x; i < ORDERED_COPIES * (n4 + 2); i += WGS) {
                float4 q = copies[i];
                const uint32_t k = i / (n4 + 2), at = i - k * (n4 + 2);
                if (at & 1) {
                    const uint2 links = at < n4 ? reinterpret_cast<const uint2*>(sv.wideNodes)[at >> 1] : make_uint2(nodeCount, nodeCount);
                    q.z = __uint_as_float(links.x);
                    q.w = __uint_as_float(links.y);
                }
                ldsScene[orderedBase + k * orderedStride + at] = q;
            }
        }
        if constexpr (LARGE) {
            /* behind the node copies, the parts HIT of a hit's data that this instantiation reads from LDS (wpt_lds_places.h has the
             * records; the host's selectLargeForm asked the same function with the same counts and launches this kernel only
             * where it says that they fit): gathered from the arrays every other kernel reads, so that the long round finds
             * there, word for word, what it would fetch from HBM */
            const uint32_t m = (args.materialsInLds & LDS_MATERIALS) ? sv.materialCount : 0u;
            const uint32_t normals = args.materialsInLds >> LDS_HIT_NORMALS_SHIFT;
            const HitDataPlaces places = hitDataPlaces(nodeCount, sv.triCount, m, normals, sv.hotspotCount, ORDERED);
            hitData.scene = ldsScene;
            hitData.corners = n4 + 2;
            hitData.recordsAt = places.recordsAt;
            hitData.hotspotsAt = places.hotspotsAt;
            hitData.normalsAt = places.normalsAt;
            if (HIT & places.parts & HIT_DATA_RECORDS) {
                for (uint32_t i = threadIdx.x; i < HIT_RECORD_QUADS * sv.triCount; i += WGS) {
                    const uint32_t tri = i / HIT_RECORD_QUADS, k = i - HIT_RECORD_QUADS * tri;
                    float4 q;
                    if (k < 6) {
                        q = sv.triAttr[6 * tri + k];
                    } else { /* instance, material, flags: the fourth words of the triangle's three records in HBM */
                        const float4* g = sv.triGeom + 3 * tri;
                        q = make_float4(g[0].w, g[1].w, g[2].w, 0.0f);
                    }
                    ldsScene[places.recordsAt + i] = q;
                }
            }
            if (HIT & places.parts & HIT_DATA_HOTSPOTS) {
                for (uint32_t i = threadIdx.x; i < HIT_HOTSPOT_QUADS * sv.hotspotCount; i += WGS) {
                    const uint32_t spot = i / HIT_HOTSPOT_QUADS, k = i - HIT_HOTSPOT_QUADS * spot;
                    const wpt_hotspot& hs = sv.hotspots[spot];
                    float4 q;
                    if (k == 0)
                        q = sv.hotspotFace[spot];
                    else if (k == 1)
                        q = make_float4(__uint_as_float(hs.prim), __uint_as_float(hs.transform), hs.p0[0], hs.p0[1]);
                    else if (k == 2)
                        q = make_float4(hs.p0[2], hs.p1[0], hs.p1[1], hs.p1[2]);
                    else if (k == 3)
                        q = make_float4(hs.p2[0], hs.p2[1], hs.p2[2], 0.0f);
                    else
                        q = make_float4(hs.M[4 * (k - 4)], hs.M[4 * (k - 4) + 1], hs.M[4 * (k - 4) + 2], hs.M[4 * (k - 4) + 3]);
                    ldsScene[places.hotspotsAt + i] = q;
                }
            }
            if (HIT & places.parts & HIT_DATA_NORMALS) {
                for (uint32_t i = threadIdx.x; i < HIT_NORMAL_QUADS * normals; i += WGS) {
                    const uint32_t instance = i / HIT_NORMAL_QUADS, k = i - HIT_NORMAL_QUADS * instance;
                    const float* N = sv.instances[instance].N;
                    ldsScene[places.normalsAt + i] = make_float4(N[3 * k], N[3 * k + 1], N[3 * k + 2], 0.0f);
                }
            }
            if constexpr ((HIT & HIT_DATA_MATERIALS) != 0) {
                /* the material records by LDS address (materialPlaces; the host asked it with the same counts): behind the
                 * corners where the copy above has put them, else behind the parts above, whole as they are in HBM */
                const bool behindCorners = (args.materialsInLds & LDS_MATERIALS) != 0;
                const MaterialPlaces mp = materialPlaces(nodeCount, sv.triCount, sv.materialCount, behindCorners, places.quads);
                hitData.materialsAt = mp.at;
                if (mp.in && !behindCorners) {
                    const float4* from = reinterpret_cast<const float4*>(sv.materials);
                    for (uint32_t i = threadIdx.x; i < HIT_MATERIAL_QUADS * sv.materialCount; i += WGS)
                        ldsScene[mp.at + i] = from[i];
                }
            }
            if constexpr ((HIT & HIT_DATA_LAUNCH) != 0) {
                /* the launch record in front of the cold words (wpt_lds_places.h; the host launches this kernel only where the
                 * scene ends in front of it): four lanes write a quadword each, and the origin is evaluated here, once */
                if (threadIdx.x < LAUNCH_RECORD_QUADS)
                    ldsScene[LAUNCH_RECORD_AT + threadIdx.x] = launchRecordQuad(threadIdx.x, args.cam, args.par, cameraOriginAtRest(args.cam), args.invWidth,
                            args.invHeight, args.invSamplesSqrt, args.samplesSqrt);
            }
        }
    }
    __syncthreads();
    auto node4 = [&](uint32_t i) -> float4 {
        if constexpr (LDSSCENE)
            return ldsScene[i];
        else
            return sv.nodes[i];
    };
    auto tri4 = [&](uint32_t i) -> float4 {
        if constexpr (LDSSCENE)
            return ldsScene[2 * nodeCount + 2 + i];
        else
            return sv.triGeom[i];
    };
    /* LDSSCENE: the node a ray's walk starts at under the launch's links (the root, or what the plan's links make of it), the
     * entry behind the null node's; rays with RAY_MAY_NAN start at the root and keep to the exact words (in sv.spheres' place) at every step */
    uint32_t walkStart = 0;
    if constexpr (LDSSCENE)
        walkStart = reinterpret_cast<const uint2*>(sv.wideNodes)[nodeCount + 1].x;

    auto pixelOf = [&](uint32_t gid, uint32_t& pixel) -> bool { return lanePixel(args, gid, pixel); };
    const bool firstPass = !ADAPTIVE && args.rowStop < args.samplesSqrt; /* (an adaptive launch is one pass) */
    const uint32_t laneLimit = args.order ? *args.orderCount : args.blockSize; /* indices a lane may take */
    /* SLICED: units per pixel and rows per unit; a launch without a pool renders every pixel in one piece */
    uint32_t sliceUnits = 1, sliceRows = 0;
    if constexpr (SLICED) {
        sliceUnits = args.pool ? args.slices.units : 1u;
        sliceRows = args.pool ? args.slices.rows : args.samplesSqrt;
    }
    FrameArgs fa;
    fa.cam = args.cam;
    fa.par = args.par;
    fa.width = args.width;
    fa.height = args.height;
    fa.samplesSqrt = args.samplesSqrt;
    fa.invWidth = args.invWidth;
    fa.invHeight = args.invHeight;
    fa.invSamplesSqrt = args.invSamplesSqrt;
    if constexpr (hasShutter(F))
        fa.shutter = args.shutter;
    /* HIT_DATA_LAUNCH: the new-sample block reads the launch's constants from the record the prologue has left in LDS (wpt_blocks.h) */
    const auto launch = [&]() {
        if constexpr ((HIT & HIT_DATA_LAUNCH) != 0)
            return LaunchRecordInLds{ ldsScene + LAUNCH_RECORD_AT };
        else
            return NoLaunchConstants{};
    }();

    /* ---- per-lane state: the pixel's path (wpt_blocks.h; its cold words in LDS) and the traversal registers ---- */
    std::conditional_t<ADAPTIVE, PathLdsSum<WG>, PathLds<WG>> ps;
    ps.base = LARGE ? ldsCold + (threadIdx.x / WG) * (SLOT_COUNT * WG) + threadIdx.x % WG : ldsCold + threadIdx.x;
    /* VIEWS: the view of the lane's pixel (the pixel's x | y << 16 fills SLOT_SRDIR.w); a register of its own */
    uint32_t view = 0;
    /* ADAPTIVE: the sample count n of the lane's pixel (0: not rendered), a register of its own; never wave-uniform */
    uint32_t laneSqrt = 0;
    /* SLICED: the lane's slot | its unit g << SLICE_SLOT_BITS, a register of its own */
    uint32_t unit = 0;
    /* the lane takes the pixel behind index `at` of the launch; false: there is none */
    auto startPixel = [&](uint32_t at) -> bool {
        uint32_t pixel = args.blockStart;
        bool have;
        if constexpr (SLICED) {
            /* unit g of the pixel behind slot at % laneLimit.  A first unit starts the pixel as ever; a later one is this lane's
             * if the lane that ran the unit before it has already left it behind (SlicesView), and then goes on from the carry */
            uint32_t g = 0, slot = at;
            if (at >= laneLimit) {
                g = at / laneLimit;
                slot = at - g * laneLimit;
            }
            have = pixelOf(slot, pixel);
            if (g > 0) {
                have = false;
                if (g < sliceUnits) {
                    const uint32_t before = __hip_atomic_fetch_or(args.slices.words + slot, 1u << (16 + g), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    have = ((before >> g) & 1u) != 0 && !(args.slices.declineOdd && (slot & 1u));
                }
            }
            unit = slot | (g << SLICE_SLOT_BITS);
            pathStateInit(ps, pixel, pixel % args.width, pixel / args.width);
            if (have && g > 0) {
                ps.base[SLOT_PRNG * WG] = args.slices.carry[2 * (size_t)slot];
                ps.base[SLOT_ACC * WG] = args.slices.carry[2 * (size_t)slot + 1];
                atomicAdd(args.slices.stats, 1ull);
            }
            return have;
        }
        if (args.order) {
            have = at < laneLimit;
            if (have)
                pixel = args.order[at];
        } else if constexpr (VIEWS) {
            /* the view, then the pixel of its frame (8x8 tiles within each view where the launch is tiled) */
            have = at < args.blockSize;
            view = have ? at / args.views.viewPixels : 0u;
            pixelOf(at - view * args.views.viewPixels, pixel);
        } else {
            have = pixelOf(at, pixel);
        }
        if constexpr (VIEWS) {
            /* the view's sample stream moves the generator's index on by whole frames, in 64 bits (ViewsView) */
            const uint64_t stream = args.views.streams ? args.views.streams[view] : 0u;
            pathStateInit(ps, (uint64_t)pixel + stream * args.views.viewPixels, pixel % args.width, pixel / args.width);
        } else {
            pathStateInit(ps, pixel, pixel % args.width, pixel / args.width);
        }
        if constexpr (ADAPTIVE) {
            laneSqrt = have ? (uint32_t)args.adaptive.samplesSqrt[pixel] : 0u;
            ps.sampleSum = mk3(0.0f, 0.0f, 0.0f);
            if (laneSqrt > 0 && args.adaptive.moments) { /* M = 0 */
                float* m = args.adaptive.moments + 3 * (size_t)pixel;
                m[0] = 0.0f;
                m[1] = 0.0f;
                m[2] = 0.0f;
            }
        }
        if (!ADAPTIVE && have && args.order) {
            /* where the first pass stopped */
            ps.base[SLOT_PRNG * WG] = args.carry[2 * (size_t)pixel];
            ps.base[SLOT_ACC * WG] = args.carry[2 * (size_t)pixel + 1];
        }
        if (have && firstPass)
            args.cost[pixel] = (uint32_t)clock64();
        return have;
    };
    const bool inBlock = startPixel(blockIdx.x * WGS + threadIdx.x);
    LaneCounters lc = LANE_COUNTERS_ZERO;
    /* wave-level scheduler statistics (COUNT builds): rounds and lane counts per state */
    unsigned long long sched[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int state = inBlock ? S_NEW : S_DONE;
    bool poolDry = false; /* wave-uniform */
    RayAux aux = rayAux(ps.d);
    /* LDSSCENE: a lane that does not walk stands on the null node (index nodeCount), and a lane that waits for its leaf test
     * keeps the leaf's index in leafNode (ldsStep below; ROTATED: the leaf's word, which says where its corners lie) */
    uint32_t node = LDSSCENE ? nodeCount : 0u, leafPrim = 0, leafNode = 0;
    float amax = k_maxval;
    /* ROTATED: the ray's origin in the order of its kz and inv[kz], beside aux, whose Sx and Sy then are the unswapped shear
     * constants and whose k is RAY_FLIP | the quadword offset of the ray's copy of the corners << 8 | RAY_MAY_NAN */
    f3 orgRotated = mk3(0.0f, 0.0f, 0.0f);
    float auxSz = 0.0f;
    /* ORDERED: the quadword offset of the ray's copy of the node array, 0 for a ray with RAY_MAY_NAN.  While such a ray walks,
     * ps.o and aux.inv hold the origin and the reciprocals with the negative axes mirrored, and bits 0 - 2 of aux.k say which
     * those are (realOrigin below) */
    uint32_t nodeCopy = 0;
    /* WIDE: the child whose turn is next (reference, entry distance) waits in registers, so that a step starts with its node's
     * fetch and not with a load from the stack; the others wait on the stack in the reference's order */
    uint2 pend[WIDE ? WIDE_STACK : 1];
    uint32_t sp = 0, curRef = WIDE_NONE;
    float curEntry = 0.0f;
    Candidate best;
    best.prim = NO_HIT;
    best.a = best.invDet = best.U = best.V = best.W = 0.0f;

    /* start the traversal of the ray ps.o, ps.d */
    auto beginRay = [&]() {
        if constexpr (ROTATED) {
            aux = rayAuxRotated(ps.d);
            const int kz = auxKz(aux);
            orgRotated = rotated(ps.o, kz);
            auxSz = comp(aux.inv, kz);
            aux.k = (aux.k & RAY_FLIP) | (int)(rotatedCopyOffset(kz, sv.triCount) << 8);
        } else {
            aux = rayAux(ps.d);
        }
        node = 0;
        amax = k_maxval;
        best.prim = NO_HIT;
        state = S_NODE;
        /* rays for which a slab distance can be NaN (a zero direction component, say) are rare; only they test for it per box,
         * and in WIDE kernels they walk the binary tree */
        if (rayMayNan(ps.o, aux.inv))
            aux.k |= RAY_MAY_NAN;
        if constexpr (LDSSCENE) {
            if (!(aux.k & RAY_MAY_NAN))
                node = walkStart;
        }
        if constexpr (ORDERED) {
            /* a ray whose slab distances are numbers walks with its negative axes mirrored (negation is exact) and reads the copy
             * of the node array that is mirrored the same way; a ray with RAY_MAY_NAN stays as it is and reads copy 0 */
            const uint32_t sign = (aux.k & RAY_MAY_NAN) ? 0u : 0x80000000u;
            const uint32_t sx = __float_as_uint(aux.inv.x) & sign, sy = __float_as_uint(aux.inv.y) & sign, sz = __float_as_uint(aux.inv.z) & sign;
            ps.o.x = __uint_as_float(__float_as_uint(ps.o.x) ^ sx);
            ps.o.y = __uint_as_float(__float_as_uint(ps.o.y) ^ sy);
            ps.o.z = __uint_as_float(__float_as_uint(ps.o.z) ^ sz);
            aux.inv.x = __uint_as_float(__float_as_uint(aux.inv.x) ^ sx);
            aux.inv.y = __uint_as_float(__float_as_uint(aux.inv.y) ^ sy);
            aux.inv.z = __uint_as_float(__float_as_uint(aux.inv.z) ^ sz);
            const uint32_t octant = (sx >> 31) | (sy >> 30) | (sz >> 29);
            aux.k |= (int)octant;
            nodeCopy = octant ? orderedBase + octant * orderedStride : 0u;
        }
        if (WIDE) {
            /* the root's wide node, admitted under any bound (the root's own box decides nothing its children do not) */
            curRef = NODE_CHILD | 0u;
            curEntry = 0.0f;
            sp = 0;
        }
        if (COUNT)
            lc.rays++;
    };
    /* state after the walk has left the tree */
    auto endOfRayState = [&]() { return ps.rayKind == RAY_PATH ? (int)S_SHADE : (int)S_NEEEND; };
    /* ORDERED: what reads ps.o behind the walk (blockShade, blockNeeEnd, finishHit) sees the ray's own origin: three sign flips
     * by the bits beginRay has left in aux.k, which are cleared so that a lane that waits in its block is not flipped twice */
    auto realOrigin = [&]() {
        if constexpr (ORDERED) {
            const uint32_t k = (uint32_t)aux.k;
            ps.o.x = __uint_as_float(__float_as_uint(ps.o.x) ^ (k << 31));
            ps.o.y = __uint_as_float(__float_as_uint(ps.o.y) ^ ((k & 2u) << 30));
            ps.o.z = __uint_as_float(__float_as_uint(ps.o.z) ^ ((k & 4u) << 29));
            aux.k &= ~7;
        }
    };
    /* what a block of wpt_blocks.h asks for next.  Rays start together at the end of the long round: the reciprocals and
     * the shear of a direction (three divisions and the axis choice, some sixty instructions) then run once for the
     * SHADE, NEE-END and NEW lanes of the round, not once behind each of their blocks. */
    auto afterBlock = [&](int next) {
        if (next == NEXT_TRACE)
            state = S_START;
        else if (next != NEXT_WAIT) /* a waiting lane keeps its state and its hit */
            state = next == NEXT_NEW ? (int)S_NEW : (int)S_DONE;
    };

    /* idle lanes take the next pixels of the launch: one atomic per wave */
    auto fromPool = [&]() {
        if (!COUNT && args.pool && !poolDry) {
            const unsigned long long idle = __ballot(state == S_DONE);
            if (idle != 0) {
                const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                const uint32_t want = (uint32_t)__popcll(idle);
                const int leader = __ffsll((long long)idle) - 1;
                uint32_t first = 0;
                if ((int)lane == leader)
                    first = atomicAdd(args.pool, want);
                first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
                if constexpr (SLICED)
                    poolDry = first + want >= sliceUnits * laneLimit; /* indices the pool hands out: every unit of every slot */
                else
                    poolDry = first + want >= laneLimit; /* the counter only grows: nothing behind it for this wave */
                if (state == S_DONE) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                    if (startPixel(first + rank))
                        state = S_NEW;
                }
            }
        }
    };

    for (;;) {
        /* ---- the wave's scheduler ----
         * Traversal (NODE steps and LEAF tests) is one block with its own inner policy; the long
         * blocks (SHADE, NEE-END, NEW) run when they are well filled, or when no traversal work
         * is left in the wave.  Waiting lanes lose nothing but time: every lane still executes
         * its own operations in order. */
        sec<COUNT>(lc, SEC_LOOK);
        const int cTrav = __popcll(__ballot(state == S_NODE || state == S_LEAF));
        const int cShade = __popcll(__ballot(state == S_SHADE));
        const int cNee = __popcll(__ballot(state == S_NEEEND));
        const int cNew = __popcll(__ballot(state == S_NEW));
        if ((cTrav | cShade | cNee | cNew) == 0)
            break;
        int pick;
        const bool fused = args.fuse != 0;
        {
            /* at least 1: a block must never be picked with no lane in it */
            const int heavyMin = (int)args.heavyMin < 1 ? 1 : (int)args.heavyMin;
            if (fused) {
                /* one long round for every lane that is not traversing: fewer lanes wait for
                 * "their" block to fill up, at the price of running up to three code sections */
                pick = (cShade + cNee + cNew >= heavyMin || cTrav == 0) ? (int)S_SHADE : (int)S_NODE;
            } else if (cShade >= heavyMin) {
                pick = S_SHADE;
            } else if (cNee >= heavyMin) {
                pick = S_NEEEND;
            } else if (cNew >= heavyMin) {
                pick = S_NEW;
            } else if (cTrav != 0) {
                pick = S_NODE;
            } else {
                int most = cShade;
                pick = S_SHADE;
                if (cNee > most) { pick = S_NEEEND; most = cNee; }
                if (cNew > most) { pick = S_NEW; most = cNew; }
            }
        }
        long long tBlock = 0;
        if (COUNT)
            tBlock = clock64();
        if constexpr (ROTATED) {
            if (pick == S_NODE) /* (the instruction takes a literal) */
                __builtin_amdgcn_s_setprio(PRIORITY_WALK);
            else
                __builtin_amdgcn_s_setprio(PRIORITY_LONG);
        }
        if (pick == S_NODE) {
            /* Leave when fewer than leaveEighths/8 of the entering lanes are still traversing
             * (never below 1: the loop must end when no lane is left in it). */
            int leaveBelow = (cTrav * (int)args.leaveEighths + 7) >> 3;
            leaveBelow = leaveBelow < 1 ? 1 : leaveBelow;
            if (COUNT)
                sched[0]++;
            /* the node a lane will test next is known one iteration ahead: its two quadwords are requested at the end
             * of the iteration before, so that the fetch runs behind the loop's ballots and branches */
            float4 pn0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pn1 = pn0;
            /* does any ray of the wave need its slab distances tested for NaN? (rays start in the long round only) */
            bool nanPossible = sv.boxesMayBeNan != 0 || __ballot((aux.k & RAY_MAY_NAN) != 0 && (state == S_NODE || state == S_LEAF)) != 0;
            /* AABB::mayHit + the stackless form of BVH::hit's walk: one node step of the lanes in state NODE (WIDE: of those among
             * them that walk the binary tree) */
                auto binaryStep = [&]() {
                if (COUNT)
                    lc.nodes++;
                const float4 n0 = PREFETCH ? pn0 : node4(2 * node), n1 = PREFETCH ? pn1 : node4(2 * node + 1);
                const uint32_t skip = __float_as_uint(n1.z);
                const uint32_t word = __float_as_uint(n1.w);
                bool hit = boxTest<false>(nodeLo(n0, n1), nodeHi(n0, n1), ps.o, aux.inv, par.min_hit_distance, amax);
                if (nanPossible) /* wave-uniform, rarely true */
                    hit = boxTest<true>(nodeLo(n0, n1), nodeHi(n0, n1), ps.o, aux.inv, par.min_hit_distance, amax);
                /* select form of: hit & inner -> first child; hit & leaf -> test it, then skip; else -> skip */
                const bool inner = word >= NODE_CHILD;
                const bool toLeaf = hit && !inner;
                leafPrim = toLeaf ? word : leafPrim;
                node = (hit && inner) ? (word & NODE_INDEX_MASK) : skip;
                state = toLeaf ? (int)S_LEAF : (int)S_NODE;
                if (!toLeaf && node >= nodeCount)
                    state = endOfRayState();
                if (PREFETCH && state == S_NODE) {
                    pn0 = node4(2 * node);
                    pn1 = node4(2 * node + 1);
                }
            };
            /* LDSSCENE: the same node step for every lane of the wave, in selects: no branch and no change of the exec mask.
             * A lane that does not walk stands on the null node, whose child and skip link are itself, and stays there; a lane
             * whose walk leaves the tree by a skip link arrives there too and keeps state NODE until the next look (below).  A lane
             * that reaches a leaf goes to the null node as well and remembers the leaf; its test reads the leaf's word and skip
             * link again -- ROTATED: it remembers the leaf's word, and the test finds the rest in the corner records.  Each
             * walking lane performs the box test and the decisions of binaryStep on the same values. */
            auto ldsStep = [&](auto nanCheck) {
                /* (ORDERED: the record of the ray's own copy; the copies' links are the same) */
                const float4 n0 = node4(2 * node + (ORDERED ? nodeCopy : 0u)), n1 = node4(2 * node + 1 + (ORDERED ? nodeCopy : 0u));
                uint32_t skip = __float_as_uint(n1.z);
                uint32_t word = __float_as_uint(n1.w); /* the LDS copy's word: child index, or ~leaf word (>= 2^31) */
                if constexpr (decltype(nanCheck)::value) {
                    /* a group in which a ray's slab distances may be NaN walks the exact links, every lane of it (node is at
                     * most nodeCount, the null node, which has its pair there too) */
                    const uint2 exact = exactLinks(sv, node);
                    skip = exact.x;
                    word = exact.y;
                }
                /* ORDERED, a group without RAY_MAY_NAN rays: every lane is mirrored to the copy it reads, so lo holds the three near
                 * bounds and hi the three far ones.  A mixed group takes the sorting test for all its lanes: a mirrored lane's
                 * pairs arrive swapped, none of its distances is NaN, and minimum and maximum do not mind the order. */
                bool hit;
                if constexpr (ORDERED && !decltype(nanCheck)::value)
                    hit = boxTestOrdered(nodeLo(n0, n1), nodeHi(n0, n1), ps.o, aux.inv, par.min_hit_distance, amax);
                else
                    hit = boxTest<decltype(nanCheck)::value>(nodeLo(n0, n1), nodeHi(n0, n1), ps.o, aux.inv, par.min_hit_distance, amax);
                const bool toLeaf = hit && (int32_t)word < 0;
                leafNode = toLeaf ? (ROTATED ? word : node) : leafNode;
                state = toLeaf ? (int)S_LEAF : state;
                node = hit ? (toLeaf ? nodeCount : word) : skip;
            };
            if (PREFETCH && state == S_NODE) {
                pn0 = node4(2 * node);
                pn1 = node4(2 * node + 1);
            }
            for (;;) {
                sec<COUNT>(lc, SEC_LOOK_INNER);
                /* LDSSCENE: a lane whose walk has left the tree in a node step takes its state after the walk here */
                if (LDSSCENE && state == S_NODE && node >= nodeCount)
                    state = endOfRayState();
                const int nNode = __popcll(__ballot(state == S_NODE));
                const int nLeaf = __popcll(__ballot(state == S_LEAF));
                if (nNode + nLeaf < leaveBelow)
                    break;
                /* The end of a light ray is a short block (its contribution, roulette, the continuation's start): lanes that
                 * wait for it do not have to wait for the long round -- once NEE_IN_WALK of them are there, the walk serves them
                 * and they walk on with the rest.  (The same block as in the long round; a lane's order of operations is its own.) */
                if (NEE_IN_WALK > 0 && !COUNT) {
                    const int nNee = __popcll(__ballot(state == S_NEEEND));
                    if (nNee >= NEE_IN_WALK) {
                        if (state == S_NEEEND)
                            afterBlock(blockNeeEnd<F>(sv, par, tri4, ps, best, args.bins));
                        if (state == S_START) {
                            beginRay();
                            if (PREFETCH) {
                                pn0 = node4(2 * node);
                                pn1 = node4(2 * node + 1);
                            }
                        }
                        nanPossible = nanPossible || __ballot((aux.k & RAY_MAY_NAN) != 0 && state == S_NODE) != 0; /* rays have started */
                        continue;
                    }
                }
                /* a leaf test is ~3 node steps long; it runs once enough lanes wait for it
                 * (leafBias/8 of the walking lanes), because waiting lanes thin out the walk */
                if (nLeaf * (int)args.leafBias >= nNode * 8 && nLeaf > 0) {
                    if (COUNT) {
                        sched[3]++;
                        sched[4] += nLeaf;
                    }
                    sec<COUNT>(lc, SEC_LEAF_TEST, state == S_LEAF);
                    if (state == S_LEAF) {
                        /* HitableTriangle::hit, candidate part (hitable_triangle.hpp:189-271); the walk already knows where
                         * it goes on (a leaf's subtree is the leaf itself) */
                        if (COUNT)
                            lc.leaves++;
                        float4 r0, r1, r2; /* ROTATED: the corners from the copy in the ray's order */
                        if constexpr (ROTATED) {
                            /* one round trip: the leaf's word says where the corners lie, and their records say the rest -- the
                             * skip link under the launch's links, the exact one (nanPossible is wave-uniform), the triangle */
                            const uint32_t at = (((uint32_t)aux.k >> 8) & 0x7fffffu) + (leafNode & LEAF_CORNER_MASK);
                            /* lgkmcnt(0) before the three reads and not between them: nothing of the walk is in flight here, but
                             * the compiler's bookkeeping across the loop's edges otherwise puts that wait behind the first read
                             * (the sliced twin), which makes the pass two round trips again */
                            __builtin_amdgcn_s_waitcnt(0xc07f);
                            r0 = tri4(at);
                            r1 = tri4(at + 1);
                            r2 = tri4(at + 2);
                            leafPrim = __float_as_uint(r2.w);
                            node = __float_as_uint(nanPossible ? r1.w : r0.w);
                            if (!(args.materialsInLds & LDS_LEAF_LINKS)) {
                                /* (a tree in which a triangle has two leaves, or none: the links of the leaf's own node) */
                                const uint32_t leaf = (leafNode >> LEAF_NODE_SHIFT) & LEAF_NODE_MAX;
                                node = nanPossible ? exactLinks(sv, leaf).x : __float_as_uint(node4(2 * leaf + 1).z);
                            }
                        } else if constexpr (LDSSCENE) {
                            /* the leaf ldsStep stopped at: its word (complemented in the LDS copy) and its skip link */
                            const float4 n1 = node4(2 * leafNode + 1);
                            leafPrim = ~__float_as_uint(n1.w);
                            node = __float_as_uint(n1.z);
                            if (nanPossible) /* wave-uniform: the exact skip link, as in ldsStep (leafNode is a leaf's index) */
                                node = exactLinks(sv, leafNode).x;
                        }
                        Candidate c;
                        bool accepted;
                        if ((F & FEAT_SPHERES) && (leafPrim & PRIM_SPHERE)) {
                            /* HitableSphere::hit (hitable_sphere.hpp:104-147) */
                            c.invDet = c.U = c.V = c.W = 0.0f;
                            accepted = sphereTest(sphereNow<F>(sv, ps, sv.spheres[leafPrim & ~PRIM_SPHERE]), ps.o, ps.d, par.min_hit_distance, amax, c.a);
                        } else if constexpr (ROTATED) {
                            /* no select by axis, and one straight run: every lane of the pass computes the whole test */
                            accepted = triangleTestRotatedStraight(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), orgRotated, aux.Sx, aux.Sy,
                                    auxSz, (uint32_t)aux.k & (uint32_t)RAY_FLIP, par.min_hit_distance, amax, c);
                        } else {
                            const float4 g0 = tri4(3 * leafPrim), g1 = tri4(3 * leafPrim + 1), g2 = tri4(3 * leafPrim + 2);
                            f3 v0 = mk3(g0.x, g0.y, g0.z), v1 = mk3(g1.x, g1.y, g1.z), v2 = mk3(g2.x, g2.y, g2.z);
                            if ((F & FEAT_ANIM) && (__float_as_uint(g2.w) & WPT_TRI_ANIMATE)) {
                                /* the instance moves: its corners at the ray's time (hitable_triangle.hpp:209-218) */
                                const float* animationM = animationMatrix(sv, ps, sv.instances[__float_as_uint(g0.w)].animation);
                                v0 = animatePoint(animationM, v0);
                                v1 = animatePoint(animationM, v1);
                                v2 = animatePoint(animationM, v2);
                            }
                            accepted = triangleTest(v0, v1, v2, ps.o, aux, par.min_hit_distance, amax, c);
                        }
                        /* WIDE: a hit whose stored distance lies beyond the bound it was accepted under (the two are separate
                         * comparisons in the reference) makes the bound grow: children dropped under the smaller bound may be
                         * due after all, so this ray starts again from the root in the binary walk */
                        const bool grown = WIDE && accepted && !(aux.k & (RAY_MAY_NAN | RAY_WALK_BINARY)) && !(c.a <= amax);
                        if constexpr (ROTATED) {
                            /* the straight test has filled c whatever it found: a rejected lane keeps its words, in selects */
                            best.prim = accepted ? leafPrim : best.prim;
                            best.a = accepted ? c.a : best.a;
                            best.invDet = accepted ? c.invDet : best.invDet;
                            best.U = accepted ? c.U : best.U;
                            best.V = accepted ? c.V : best.V;
                            best.W = accepted ? c.W : best.W;
                            amax = accepted ? c.a : amax;
                        } else if (accepted) {
                            c.prim = leafPrim;
                            best = c;
                            amax = c.a;
                        }
                        if (WIDE && !(aux.k & (RAY_MAY_NAN | RAY_WALK_BINARY)))
                            state = curRef == WIDE_NONE ? endOfRayState() : (int)S_NODE;
                        else
                            state = node >= nodeCount ? endOfRayState() : (int)S_NODE;
                        /* A light ray towards the environment asks one thing: is anything in the way (blockNeeEnd,
                         * wurblpt.hpp:240-250).  Up to a walk's first accepted hit the bound is the ray's own, so every box
                         * and leaf decision is the reference's, and the answer is known there: the walk ends.  (Counting
                         * launches are given shadowWalksEnd = 0 and walk on, as the reference does: their numbers are its numbers.) */
                        if ((F & FEAT_ENVMAP) && args.shadowWalksEnd && accepted && ps.rayKind == RAY_NEE_ENV) {
                            state = S_NEEEND;
                            if (LDSSCENE)
                                node = nodeCount;
                        } else if (grown) {
                            aux.k |= RAY_WALK_BINARY;
                            node = 0;
                            amax = k_maxval;
                            best.prim = NO_HIT;
                            state = S_NODE;
                        }
                        if (PREFETCH && state == S_NODE) {
                            pn0 = node4(2 * node);
                            pn1 = node4(2 * node + 1);
                        }
                    }
                } else {
                    if (COUNT) {
                        sched[1]++;
                        sched[2] += nNode;
                    }
                    if constexpr (WIDE) {
                        if (state == S_NODE && !(aux.k & (RAY_MAY_NAN | RAY_WALK_BINARY))) {
                            /* The child whose turn it is: admitted if its entry distance is within the bound of this moment
                             * (the reference's test at its turn); a leaf goes to its test, an inner node's four entries are
                             * tested under the bound, the first the ray passes through is next, the others wait on the stack in
                             * the reference's order.  The stack's top is requested before the node, so that it is there when no
                             * entry of this step is next. */
                            const uint32_t ref = curRef;
                            const bool admitted = curEntry <= amax;
                            uint2 top = make_uint2(WIDE_NONE, 0u);
                            if (sp > 0)
                                top = pend[sp - 1];
                            curRef = WIDE_NONE;
                            if (admitted && ref < NODE_CHILD) {
                                leafPrim = ref;
                                state = S_LEAF;
                            } else if (admitted) {
                                const float4* w = sv.wideNodes + 8 * (size_t)(ref & NODE_INDEX_MASK);
                                const float4 lx = w[0], ly = w[1], lz = w[2], hx = w[3], hy = w[4], hz = w[5], rf = w[6];
                                const float amin = par.min_hit_distance;
                                /* entries 3, 2, 1, 0: the last one that passes (the first in the reference's order) stays in
                                 * registers, the one it displaces goes to the stack */
                                auto entryOf = [&](float lox, float loy, float loz, float hix, float hiy, float hiz, uint32_t r) {
                                    const float t0x = (lox - ps.o.x) * aux.inv.x, t0y = (loy - ps.o.y) * aux.inv.y, t0z = (loz - ps.o.z) * aux.inv.z;
                                    const float t1x = (hix - ps.o.x) * aux.inv.x, t1y = (hiy - ps.o.y) * aux.inv.y, t1z = (hiz - ps.o.z) * aux.inv.z;
                                    const float near = __builtin_fmaxf(__builtin_fmaxf(amin, __builtin_fminf(t0x, t1x)),
                                            __builtin_fmaxf(__builtin_fminf(t0y, t1y), __builtin_fminf(t0z, t1z)));
                                    const float far = __builtin_fminf(__builtin_fminf(amax, __builtin_fmaxf(t0x, t1x)),
                                            __builtin_fminf(__builtin_fmaxf(t0y, t1y), __builtin_fmaxf(t0z, t1z)));
                                    if (r != WIDE_NONE && near <= far) {
                                        if (curRef != WIDE_NONE)
                                            pend[sp++] = make_uint2(curRef, __float_as_uint(curEntry));
                                        curRef = r;
                                        curEntry = near;
                                    }
                                };
                                entryOf(lx.w, ly.w, lz.w, hx.w, hy.w, hz.w, __float_as_uint(rf.w));
                                entryOf(lx.z, ly.z, lz.z, hx.z, hy.z, hz.z, __float_as_uint(rf.z));
                                entryOf(lx.y, ly.y, lz.y, hx.y, hy.y, hz.y, __float_as_uint(rf.y));
                                entryOf(lx.x, ly.x, lz.x, hx.x, hy.x, hz.x, __float_as_uint(rf.x));
                            }
                            if (curRef == WIDE_NONE && top.x != WIDE_NONE) { /* nothing of this step is next: the stack's top is */
                                curRef = top.x;
                                curEntry = __uint_as_float(top.y);
                                sp--;
                            }
                            if (state == S_NODE && curRef == WIDE_NONE)
                                state = endOfRayState();
                        }
                        /* the few rays that walk the binary tree (a NaN slab distance is possible, or the bound has grown) */
                        if (__ballot(state == S_NODE && (aux.k & (RAY_MAY_NAN | RAY_WALK_BINARY))) != 0) {
                            if (state == S_NODE && (aux.k & (RAY_MAY_NAN | RAY_WALK_BINARY)))
                                binaryStep();
                        }
                    } else if constexpr (LDSSCENE) {
                        static_assert(!COUNT, "the LDS kernel has no counting build: ldsStep counts nothing");
                        /* nanPossible is uniform and does not change within the block (no light-ray ends in this walk) */
                        if (nanPossible) {
#pragma unroll
                            for (int step = 0; step < STEPS; step++)
                                ldsStep(std::true_type());
                        } else {
#pragma unroll
                            for (int step = 0; step < STEPS; step++)
                                ldsStep(std::false_type());
                        }
                    } else {
#pragma unroll
                        for (int step = 0; step < STEPS; step++) {
                            sec<COUNT>(lc, SEC_NODE_STEP, state == S_NODE);
                            if (state == S_NODE)
                                binaryStep();
                        }
                    }
                }
            }
        }
        if (COUNT && pick == S_NODE)
            sched[11] += (unsigned long long)(clock64() - tBlock);
        if (pick != S_NODE && (fused ? cShade > 0 : pick == S_SHADE)) {
            if (COUNT) {
                tBlock = clock64();
                sched[5]++;
                sched[6] += cShade;
            }
            if (state == S_SHADE) { /* tracePath, one path component (wurblpt.hpp:131-252) */
                realOrigin();
                /* (the large form's blocks find a triangle by hitData, which knows the hit's data in LDS besides the corners) */
                if constexpr (LARGE)
                    afterBlock(blockShade<F, COUNT>(sv, par, hitData, ps, best, lc, cTrav != 0 ? (int)args.waitBelow : 0, args.bins));
                else
                    afterBlock(blockShade<F, COUNT>(sv, par, tri4, ps, best, lc, cTrav != 0 ? (int)args.waitBelow : 0, args.bins));
            }
            if (COUNT)
                sched[12] += (unsigned long long)(clock64() - tBlock);
        }
        if (pick != S_NODE && (fused ? cNee > 0 : pick == S_NEEEND)) {
            if (COUNT) {
                tBlock = clock64();
                sched[7]++;
                sched[8] += cNee;
            }
            sec<COUNT>(lc, SEC_NEE_END, state == S_NEEEND);
            sec<COUNT>(lc, SEC_NEE_END_LIGHT, state == S_NEEEND && ps.rayKind == RAY_NEE_LIGHT && best.prim == ps.getW(SLOT_NEE));
            if (state == S_NEEEND) { /* the next-event ray's contribution, then the path continues */
                realOrigin();
                if constexpr (LARGE)
                    afterBlock(blockNeeEnd<F>(sv, par, hitData, ps, best, args.bins));
                else
                    afterBlock(blockNeeEnd<F>(sv, par, tri4, ps, best, args.bins));
            }
            if (COUNT)
                sched[13] += (unsigned long long)(clock64() - tBlock);
        }
        /* last: in a fused round it also serves the lanes whose path has just ended above */
        if (pick != S_NODE && (fused ? __ballot(state == S_NEW) != 0 : pick == S_NEW)) {
            if (COUNT) {
                tBlock = clock64();
                sched[9]++;
                sched[10] += __popcll(__ballot(state == S_NEW));
            }
            sec<COUNT>(lc, SEC_NEW_SAMPLE, state == S_NEW);
            if (state == S_NEW) { /* the pixel's next sample (wurblpt.hpp:348-360), or nothing more */
                const bool passEnds = firstPass && (ps.getW(SLOT_ACC) >> 16) >= args.rowStop;
                int next;
                if constexpr (SLICED) {
                    /* the lane's unit ends where the pixel's next row of strata is the next unit's first */
                    const uint32_t g = unit >> SLICE_SLOT_BITS;
                    const uint32_t rowEnd = (g + 1) * sliceRows < args.samplesSqrt ? (g + 1) * sliceRows : args.samplesSqrt;
                    next = (ps.getW(SLOT_ACC) >> 16) >= rowEnd ? (int)NEXT_DONE : blockNew<F>(fa, ps, sv, launch);
                    if (next == NEXT_DONE && rowEnd < args.samplesSqrt) {
                        /* not the pixel's last: leave generator and sum behind, then say so.  Whoever drew the next unit before
                         * this moment has passed it by: then it is this lane's, which has the pixel's state where it is */
                        const uint32_t slot = unit & SLICE_SLOT_MASK;
                        args.slices.carry[2 * (size_t)slot] = ps.base[SLOT_PRNG * WG];
                        args.slices.carry[2 * (size_t)slot + 1] = ps.base[SLOT_ACC * WG];
                        const uint32_t before = __hip_atomic_fetch_or(args.slices.words + slot, 1u << (g + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                        next = NEXT_HANDED_ON; /* the lane is done with it, and nothing of it goes to the frame yet */
                        if (((before >> (17 + g)) & 1u) != 0 || (args.slices.declineOdd && (slot & 1u))) {
                            unit += 1u << SLICE_SLOT_BITS;
                            atomicAdd(args.slices.stats + 1, 1ull);
                            next = NEXT_NEW; /* its first sample starts with the wave's next long round */
                        }
                    }
                } else if constexpr (ADAPTIVE) {
                    /* a sample has ended unless the pixel is at its first stratum: M += S * S, then S = 0 */
                    const f3 s = ps.sampleSum;
                    if (args.adaptive.moments && ps.getW(SLOT_ACC) != 0) {
                        const uint32_t pxy = ps.getW(SLOT_SRDIR);
                        float* m = args.adaptive.moments + 3 * ((size_t)(pxy >> 16) * args.width + (pxy & 0xffffu));
                        m[0] = m[0] + s.x * s.x;
                        m[1] = m[1] + s.y * s.y;
                        m[2] = m[2] + s.z * s.z;
                    }
                    ps.sampleSum = mk3(0.0f, 0.0f, 0.0f);
                    /* the lane's own sample count: 1.0f / (float)n divided here is the host's division bit for bit */
                    FrameArgs fl = fa;
                    fl.samplesSqrt = laneSqrt;
                    fl.invSamplesSqrt = 1.0f / (float)laneSqrt;
                    next = blockNew<F>(fl, ps, sv);
                } else if constexpr (VIEWS) {
                    /* Camera::getRay from the lane's own view: scalar reads of one camera where the lanes here are all on
                     * one view (a wave in the middle of a view), each lane's own camera where they are not */
                    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)view);
                    if (passEnds)
                        next = NEXT_DONE;
                    else if (__ballot(view != first) == 0)
                        next = blockNewFrom<F, true>(fa, args.views.cams[first], ps, sv);
                    else
                        next = blockNewFrom<F, false>(fa, args.views.cams[view], ps, sv);
                } else {
                    next = passEnds ? (int)NEXT_DONE : blockNew<F>(fa, ps, sv, launch);
                }
                sec<COUNT>(lc, SEC_PIXEL_DONE, next == NEXT_DONE);
                if (next == NEXT_DONE) {
                    const uint32_t pxy = ps.getW(SLOT_SRDIR);
                    /* VIEWS: the pixel's index in the batch's frames */
                    const size_t at = (VIEWS ? (size_t)view * args.views.viewPixels : 0u) + (size_t)(pxy >> 16) * args.width + (pxy & 0xffffu);
                    if (firstPass) {
                        args.carry[2 * at] = ps.base[SLOT_PRNG * WG];
                        args.carry[2 * at + 1] = ps.base[SLOT_ACC * WG];
                        args.cost[at] = (uint32_t)clock64() - args.cost[at];
                    } else if (ADAPTIVE) {
                        /* finishPixel with the pixel's own 1 / n^2 (the unsigned product converted, as mcpt() does); a pixel
                         * with n = 0 keeps what its entries held */
                        if (laneSqrt > 0) {
                            const float invSamples = 1.0f / (float)(laneSqrt * laneSqrt);
                            const Slot acc = ps.get(SLOT_ACC);
                            float* out = args.frame + 3 * at;
                            out[0] = invSamples * acc.x;
                            out[1] = invSamples * acc.y;
                            out[2] = invSamples * acc.z;
                            if (args.adaptive.moments) {
                                float* m = args.adaptive.moments + 3 * at;
                                m[0] = invSamples * m[0];
                                m[1] = invSamples * m[1];
                                m[2] = invSamples * m[2];
                            }
                        }
                    } else if (!(F & (FEAT_TRANSIENT | FEAT_TOF)) || args.frame) {
                        /* SensorRGB::finishPixel (sensor_rgb.hpp:82-87) */
                        const Slot acc = ps.get(SLOT_ACC);
                        float* out = args.frame + 3 * at;
                        out[0] = args.invSamples * acc.x;
                        out[1] = args.invSamples * acc.y;
                        out[2] = args.invSamples * acc.z;
                    }
                }
                afterBlock(next);
            }
            fromPool();
            if (COUNT) /* shader clock spent per kind of block: [11] traversal [12] shade [13] nee-end [14] new */
                sched[14] += (unsigned long long)(clock64() - tBlock);
        }
        if (pick != S_NODE) {
            sec<COUNT>(lc, SEC_BEGIN_RAY, state == S_START);
            if (state == S_START)
                beginRay();
        }
    }

    if (COUNT && args.counters && inBlock) {
        atomicAdd((unsigned long long*)&args.counters->samples, (unsigned long long)args.samplesSqrt * args.samplesSqrt);
        atomicAdd((unsigned long long*)&args.counters->rays, (unsigned long long)lc.rays);
        atomicAdd((unsigned long long*)&args.counters->node_visits, (unsigned long long)lc.nodes);
        atomicAdd((unsigned long long*)&args.counters->leaf_tests, (unsigned long long)lc.leaves);
        atomicAdd((unsigned long long*)&args.counters->pdf_tests, (unsigned long long)lc.pdfs);
        atomicAdd((unsigned long long*)&args.counters->scatters, (unsigned long long)lc.scatters);
    }
    if (COUNT && args.schedStats && (threadIdx.x & 63) == 0) {
        for (int i = 0; i < 16; i++)
            atomicAdd(args.schedStats + i, sched[i]);
    }
    if (COUNT && args.schedStats && inBlock) { /* [16..23]: lane-weighted clock per section of the SHADE block */
        for (int i = 0; i < 8; i++)
            atomicAdd(args.schedStats + 16 + i, lc.shadeClock[i]);
    }
    if (COUNT && args.schedStats) { /* [24 ..]: executions of each stretch of code by waves, then by lanes (SEC_COUNT each) */
        for (int i = 0; i < SEC_COUNT; i++) {
            if (lc.secWave[i])
                atomicAdd(args.schedStats + 24 + i, (unsigned long long)lc.secWave[i]);
            if (lc.secLane[i])
                atomicAdd(args.schedStats + 24 + SEC_COUNT + i, (unsigned long long)lc.secLane[i]);
        }
    }
