/*
 * wpt_capi_render.hip -- of include/wurblpt_hip.h: wpt_render_block(_device) and wpt_render_bands(_device), the same four with a
 * rolling shutter (wpt_render_shutter_*, wpt_shutter_row_interval, wpt_shutter_span; wpt_shutter.h), and behind them the
 * one launch of the path tracer that every sensor and every stage of a session goes through: check, set up, choose the kernel
 * (wpt_kernel_table.h), plan its passes (wpt_launch_plan.h), execute -- the single kernel by the plan's strategy, or the
 * wavefront form (wpt_wavefront.inc.h).  The kernel itself is in wpt_pathtrace.inc.h.
 */
#include <atomic>

#include "wpt_capi_common.h"
#include "wpt_leaf_words.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

namespace {

/* the two counters of the sliced kernels (wpt_last_slice_stats), one pair per device, allocated at a device's first sliced
 * launch and kept */
constexpr int SLICE_STATS_DEVICES = 64;
std::atomic<unsigned long long*> g_sliceStats[SLICE_STATS_DEVICES];

unsigned long long* sliceStatsOfCurrentDevice()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SLICE_STATS_DEVICES)
        return nullptr;
    unsigned long long* p = g_sliceStats[dev].load(std::memory_order_acquire);
    if (!p) {
        if (hipMalloc(reinterpret_cast<void**>(&p), 2 * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        unsigned long long* expected = nullptr;
        if (!g_sliceStats[dev].compare_exchange_strong(expected, p, std::memory_order_acq_rel)) {
            (void)hipFree(p);
            p = expected;
        }
    }
    return p;
}

/* the single kernel of a launch, as every execution below launches it */
struct SingleKernel {
    void (*launch)(const wptk::KernelArgs&, dim3 grid, size_t sceneLdsBytes, hipStream_t);
    dim3 grid;
    size_t sceneLdsBytes;
    hipStream_t stream;
    void operator()(const wptk::KernelArgs& a) const { launch(a, grid, sceneLdsBytes, stream); }
};

/* TWO_PASSES: one timed row of strata of every pixel, then the rest in the order of those times.  false, and nothing
 * launched: the memory cannot be had. */
bool runTwoPasses(const wptk::KernelArgs& args, const SingleKernel& run, StreamScratch& scratch)
{
    const size_t pixels = size_t(args.width) * args.height;
    float4* carry;
    uint32_t *cost, *order, *work;
    if (!(carry = scratch.get<float4>(pixels * 2)) || !(cost = scratch.get<uint32_t>(pixels)) || !(order = scratch.get<uint32_t>(args.blockSize))
            || !(work = scratch.get<uint32_t>(ORDER_WORK_WORDS)))
        return false;
    wptk::KernelArgs first = args, second = args;
    first.rowStop = 1;
    first.carry = second.carry = carry;
    first.cost = cost;
    run(first);
    orderByCost(first, order, work, run.stream, second);
    run(second);
    return true;
}

/* ADAPTIVE_ORDER: one pass in the order built from the sample counts n^2 of the map.  false as above. */
bool runAdaptiveOrder(const wptk::KernelArgs& args, const SingleKernel& run, StreamScratch& scratch)
{
    uint32_t *cost, *order, *work;
    if (!(cost = scratch.get<uint32_t>(args.blockSize)) || !(order = scratch.get<uint32_t>(args.blockSize)) || !(work = scratch.get<uint32_t>(ORDER_WORK_WORDS)))
        return false;
    wptk::KernelArgs measure = args, ordered = args;
    measure.cost = cost - args.blockStart; /* indexed by the frame's pixel: the block's pixels land in the allocation */
    wptk::launchAdaptiveCost(measure, run.stream);
    orderByCost(measure, order, work, run.stream, ordered);
    run(ordered);
    return true;
}

/* SLICED: one launch of the kernel's twin that hands the pixels out in plan.units units of plan.rows rows.  Returns the
 * counters the launch adds to (wpt_last_slice_stats), or NULL and nothing launched: they or the memory cannot be had. */
unsigned long long* runSliced(const wptk::KernelArgs& args, const SingleKernel& runTwin, const wptk::LaunchPlan& plan, StreamScratch& scratch)
{
    unsigned long long* stats = sliceStatsOfCurrentDevice();
    float4* carry;
    uint32_t* words;
    if (!stats || !(carry = scratch.get<float4>(size_t(args.blockSize) * 2)) || !(words = scratch.get<uint32_t>(args.blockSize)))
        return nullptr;
    if (hipMemsetAsync(words, 0, size_t(args.blockSize) * sizeof(uint32_t), runTwin.stream) != hipSuccess
            || hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), runTwin.stream) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    wptk::KernelArgs inSlices = args;
    inSlices.slices = { words, carry, stats, plan.rows, plan.units, (settings.slices & WPT_SLICES_DECLINE_ODD) ? 1u : 0u };
    runTwin(inSlices);
    return stats;
}

} /* namespace */

namespace wptc {

/* The frame and block checks of every render call, one text each.  samplesSqrt: NULL where the call has none (an adaptive map
 * holds the counts); the block must lie in `frames` frames of width * height pixels (a batch of views: one per camera); prefix:
 * what the entry point's messages begin with; session: an empty block is refused too. */
wpt_status checkFrameBlock(uint32_t width, uint32_t height, const uint32_t* samplesSqrt, uint32_t blockStart, uint32_t blockSize,
        uint32_t frames, const char* prefix, bool session)
{
    if (width == 0 || height == 0 || width > 65535 || height > 65535 || (samplesSqrt && (*samplesSqrt == 0 || *samplesSqrt > 65535)))
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(prefix) + (samplesSqrt ? "width, height and samples_sqrt" : "width and height")
                + " must lie in 1 .. 65535");
    /* (width * height fits 32 bits after the check above) */
    if ((session && blockSize == 0) || uint64_t(blockStart) + blockSize > uint64_t(width) * height * frames)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(prefix) + (session ? "pixel block is empty or lies outside the frame"
                : "pixel block lies outside the frame"));
    return WPT_OK;
}

/* What every launch of the single kernel sets up the same way, a plain block, bands, a batch of views or a stage of a session
 * (wpt_progress_begin): the frame's constants, the 8x8 tiles, the features the cameras add to the scene's, the scheduler's
 * settings.  `camera` is the first of cameraCount cameras (batch: they are a batch of views); frame, counters, the sensor's
 * view and what a stage adds are the caller's. */
wpt_status launchSetUp(const wpt_scene* scene, const wpt_camera* camera, uint32_t cameraCount, bool batch, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        uint32_t band_pixels, uint32_t band_first, uint32_t band_stride, bool count, wptk::KernelArgs& args, uint32_t& need)
{
    args.bandPixels = band_pixels;
    args.bandFirst = band_first;
    args.bandStride = band_stride;
    args.sv = scene->view;
    args.cam = *camera;
    args.par = *params;
    args.width = width;
    args.height = height;
    args.samplesSqrt = samples_sqrt;
    args.invWidth = 1.0f / float(width);
    args.invHeight = 1.0f / float(height);
    args.invSamplesSqrt = 1.0f / float(samples_sqrt);
    args.invSamples = 1.0f / float(samples_sqrt * samples_sqrt);
    args.blockStart = block_start;
    args.blockSize = block_size;
    args.fuse = (settings.variant & 0x20u) ? 0u : 1u; /* variant bit 0x20: separate SHADE / NEE-END / NEW rounds (the older scheduler) */

    /* a wave covers an 8x8 pixel tile when the block consists of whole groups of 8 rows */
    args.tiled = (width % 8 == 0 && block_start % width == 0 && block_size % (8 * width) == 0
            && (band_stride == 0 || band_pixels % (8 * width) == 0)) ? 1u : 0u;
    if (batch) /* 8x8 tiles within each view's frame */
        args.tiled = (width % 8 == 0 && height % 8 == 0) ? 1u : 0u;
    /* a batch takes the union of the scene's features and every camera's */
    need = scene->features;
    for (uint32_t v = 0; v < cameraCount; v++) {
        const wpt_camera* c = camera + v;
        need |= (c->lens_radius > 0.0f || c->distortion_type != WPT_DISTORTION_NONE || c->surround_mode != WPT_SURROUND_OFF
                || c->stereoscopic_distance > 0.0f) ? FEAT_LENS : 0u;
        if (c->surround_mode > WPT_SURROUND_360)
            return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
        if (c->distortion_type > WPT_DISTORTION_OPENCV)
            return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
        if (c->animation >= int32_t(scene->animationCount))
            return fail(WPT_ERR_INVALID_ARGUMENT, batch ? "camera " + std::to_string(v) + " refers to an animation outside the scene's array"
                    : std::string("camera refers to an animation outside the scene's array"));
        if (batch && c->animation >= 0) /* an animated camera selects the moving-scene kernels */
            need |= FEAT_ANIM;
    }
    /* an exposure interval changes every path (each camera ray draws its time), moving instances need the time too */
    if (params->t0 != params->t1)
        need |= FEAT_ANIM;
    /* The walk of a light ray towards the environment ends at its first accepted hit (wpt_pathtrace.inc.h: the answer it is
     * traced for is known there).  Counting launches walk on as the reference does, so that their counters are the
     * reference's; measurements (wpt_set_walk): WPT_WALK_COUNT_PRODUCT makes them count what the product kernel walks,
     * WPT_WALK_FULL_SHADOW switches the short cut off everywhere. */
    args.shadowWalksEnd = (settings.walk & WPT_WALK_FULL_SHADOW) ? 0u : (count ? ((settings.walk & WPT_WALK_COUNT_PRODUCT) ? 1u : 0u) : 1u);
    /* scheduler defaults from sweeps on the Cornell box (scene in LDS, short walks) and on the
     * Sponza-class scene (deep tree in HBM: traversal dominates, so long blocks may run with fewer
     * lanes and leaf tests earlier) */
    const bool smallScene = size_t(scene->nodeCount) * 32 + size_t(scene->triCount) * 48 <= LDS_SCENE_MAX_BYTES;
    /* clamped: with more than 8 eighths the traversal block would leave before doing anything */
    args.leaveEighths = settings.leaveEighths ? (settings.leaveEighths > 8u ? 8u : settings.leaveEighths) : (smallScene ? 1u : 3u);
    args.heavyMin = settings.heavyMin ? settings.heavyMin : (smallScene ? 16u : 8u);
    args.leafBias = settings.leafBias ? settings.leafBias : (smallScene ? 16u : 32u);
    /* variant bits 2-3: 0 = default, 1 = no kind of material ever stands back, 2 / 3 = fewer than 3 / 12 lanes */
    static const uint32_t waitBelowChoices[4] = { 6u, 0u, 3u, 12u };
    args.waitBelow = waitBelowChoices[(settings.variant >> 2) & 0x3u];
    args.cuCount = uint32_t(scene->cuCount);
    return WPT_OK;
}

/* The single kernel by the plan's strategy, and the pool's counter where the plan has one.  Where the memory a strategy needs
 * cannot be had (the counter first of all), one plain pass renders the launch.  Returns the launch's error. */
hipError_t runSingleKernel(const wpt_scene* scene, wptk::KernelArgs& args, const wptk::KernelChoice& choice, const wptk::KernelEntry* kernel,
        const wptk::KernelEntry* slicedTwin, const wptk::LaunchPlan& plan, hipStream_t stream)
{
    StreamScratch scratch(stream);
    args.pool = plan.pooled ? scratch.get<uint32_t>(1) : nullptr;
    args.materialsInLds = choice.materialsInLds;
    if (choice.ldsScene) {
        /* The link words of the tree's copy in LDS.  Exact: the fold's, or every node's own under WPT_WALK_NO_FOLD; the launch's:
         * the ones that go round the nodes the scene's plan leaves out -- they are built on the fold, so not under NO_FOLD, not
         * under WPT_WALK_NO_BYPASS, and not for a tree with a NaN bound, whose rays all keep the exact links. */
        if (!scene->ldsLinks)
            return hipErrorInvalidValue; /* (every scene that fits LDS has them) */
        const size_t words = 2 * size_t(scene->nodeCount) + 4;
        const bool fold = (choice.materialsInLds & wptk::LDS_FOLD) != 0;
        const bool bypass = fold && !(settings.walk & WPT_WALK_NO_BYPASS) && !args.sv.boxesMayBeNan;
        args.sv.spheres = reinterpret_cast<const wpt_sphere*>(scene->ldsLinks + (fold ? words : 0));
        args.sv.wideNodes = reinterpret_cast<const float4*>(scene->ldsLinks + (bypass ? 2 * words : fold ? words : 0));
        if (choice.rotated) {
            /* the same sets with the leaf words of the rotated kernels (wpt_leaf_words.h) */
            const size_t leafWords = wptw::leafWordsSize(scene->nodeCount, scene->triCount);
            const uint32_t* sets = scene->ldsLinks + 3 * words;
            args.sv.spheres = reinterpret_cast<const wpt_sphere*>(sets + (fold ? leafWords : 0));
            args.sv.wideNodes = reinterpret_cast<const float4*>(sets + (bypass ? 2 * leafWords : fold ? leafWords : 0));
            if (scene->leafOneToOne)
                args.materialsInLds |= wptk::LDS_LEAF_LINKS;
        }
    }
    /* the large form of the kernel with rotated corners and of its twin, where the launch can take it (wpt_kernel_table.h) */
    size_t largeLdsBytes = 0;
    uint32_t hitData = 0; /* ... and what of a hit's data it keeps in LDS behind the node copies (wpt_lds_places.h) */
    const bool large = wptk::selectLargeForm(choice, settings.walk, scene->orderedNodes != nullptr, args.sv.boxesMayBeNan != 0, scene->nodeCount,
            { scene->triCount, args.sv.materialCount, scene->normalsNamed, args.sv.hotspotCount }, &largeLdsBytes, &hitData);
    if (large && wptk::LARGE_ORDERED)
        args.sv.rglData = reinterpret_cast<const float*>(scene->orderedNodes); /* (the kernel reads the copies there) */
    if (large)
        args.materialsInLds |= hitData;
    const SingleKernel run = large
            ? SingleKernel{ wptk::launchPathtraceLarge<FEAT_BASIC | FEAT_ROTATED>, dim3((args.blockSize + WG_LARGE - 1) / WG_LARGE), largeLdsBytes, stream }
            : SingleKernel{ kernel->launch, dim3((args.blockSize + WG - 1) / WG), choice.sceneLdsBytes, stream };
    bool done = false;
    unsigned long long* sliceStats = nullptr;
    if (args.pool && plan.strategy == wptk::TWO_PASSES)
        done = runTwoPasses(args, run, scratch);
    else if (args.pool && plan.strategy == wptk::ADAPTIVE_ORDER)
        done = runAdaptiveOrder(args, run, scratch);
    else if (args.pool && plan.strategy == wptk::SLICED)
        done = (sliceStats = runSliced(args, SingleKernel{ large ? wptk::launchPathtraceLarge<FEAT_BASIC | FEAT_ROTATED | FEAT_SLICED> : slicedTwin->launch, run.grid, run.sceneLdsBytes, stream },
                plan, scratch)) != nullptr;
    if (!done)
        run(args);
    recordLaunch(kernel->name, kernelForm(choice.rotated, sliceStats ? plan.units : 0, choice.rotated && !scene->leafOneToOne), done ? plan.passes : 1u,
            sliceStats);
    if (large)
        recordWorkgroup(WG_LARGE, wptk::LARGE_ORDERED, (hitData >> wptk::LDS_HIT_DATA_SHIFT) & 7u,
                ((hitData >> wptk::LDS_HIT_DATA_SHIFT) & wptk::HIT_DATA_MATERIALS) != 0, ((hitData >> wptk::LDS_HIT_DATA_SHIFT) & wptk::HIT_DATA_LAUNCH) != 0);
    return hipGetLastError();
}

/* one launch, in five steps: check, set up, choose the kernel (wpt_kernel_table.h), plan its passes (wpt_launch_plan.h), execute */
wpt_status renderLaunch(const LaunchRequest& rq)
{
    const bool planes = rq.sensor == wptk::SENSOR_TRANSIENT || rq.sensor == wptk::SENSOR_TOF, views = rq.sensor == wptk::SENSOR_VIEWS;
    if (!rq.scene || !rq.camera || !rq.params || !(rq.frame || planes))
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const uint32_t cameraCount = views ? rq.views.viewCount : 1u;
    const wpt_status checked = checkFrameBlock(rq.width, rq.height, &rq.samplesSqrt, rq.blockStart, rq.bandStride ? 0u : rq.blockSize, cameraCount);
    if (checked != WPT_OK || rq.blockSize == 0)
        return checked;
    KernelArgs args = {};
    uint32_t need = 0;
    const bool count = rq.counters != nullptr;
    WPT_TRY(launchSetUp(rq.scene, rq.camera, cameraCount, views, rq.params, rq.width, rq.height, rq.samplesSqrt, rq.blockStart,
            rq.blockSize, rq.bandPixels, rq.bandFirst, rq.bandStride, count, args, need));
    args.frame = rq.frame;
    args.counters = rq.counters;
    args.schedStats = settings.schedStats;
    if (views)
        args.views = rq.views;
    else if (rq.sensor == wptk::SENSOR_ADAPTIVE)
        args.adaptive = rq.adaptive;
    else if (planes)
        args.bins = rq.bins;
    else if (rq.sensor == wptk::SENSOR_FRAME)
        args.shutter = rq.shutter;
    /* rows read out at different times are a moving scene's business even where nothing else moves: each ray carries its row's
     * time.  (A shutter with row_time == 0 is the plain launch, kernel and all.) */
    if (rq.sensor == wptk::SENSOR_FRAME && rq.shutter.rowTime != 0.0f)
        need |= FEAT_ANIM;
    args.rowStop = rq.samplesSqrt;
    const wptk::KernelChoice choice = wptk::selectKernel({ need, rq.sensor, count, rq.scene->nodeCount, rq.scene->triCount,
            uint32_t(rq.scene->view.materialCount), rq.scene->view.wideNodes != nullptr, settings.variant, settings.walk });
    const wptk::KernelEntry *kernel = nullptr, *slicedTwin = nullptr;
    wpt_status found = lookupKernel(choice.features, choice.count, choice.ldsScene, choice.wide, &kernel);
    /* its twin that hands pixels out in slices, for a SLICED plan */
    if (found == WPT_OK && choice.sceneInLds && rq.sensor == wptk::SENSOR_FRAME && !count)
        found = lookupKernel(choice.features | FEAT_SLICED, choice.count, choice.ldsScene, choice.wide, &slicedTwin);
    if (found != WPT_OK)
        return found;
    const bool rgl = (need & FEAT_RGL) != 0;
    hipStream_t stream = static_cast<hipStream_t>(rq.stream);
    const wptk::LaunchPlan plan = wptk::planLaunch({ rq.sensor, count, rgl, (need & FEAT_ANIM) != 0, choice.sceneInLds, rq.blockSize, rq.samplesSqrt,
            uint32_t(rq.scene->cuCount), settings.variant, settings.wfMode, settings.slices });
    if (plan.wavefront) {
        uint32_t launches = 0; /* of trace and shade, two kernels that hand rays through HBM (wpt_wavefront.inc.h) */
        const hipError_t e = wptk::renderWavefront(args, rgl ? wptk::wfFullRgl() : (choice.basic ? wptk::wfBasic() : wptk::wfFull()), settings.wfConfig, stream, &launches);
        if (e == hipSuccess) {
            recordLaunch("wf_trace + wf_shade", "", launches, nullptr);
            return WPT_OK;
        }
        /* the library's own choice must not fail where the single kernel would not: without the memory for the records (256 B
         * per lane) that one renders the frame; a forced wavefront render reports the error */
        if (!plan.wavefrontFallBack || e != hipErrorOutOfMemory)
            return hipStatus("wavefront render", e, true);
        (void)hipGetLastError();
    }
    HIP_TRY(runSingleKernel(rq.scene, args, choice, kernel, slicedTwin, plan, stream));
    return WPT_OK;
}

} /* namespace wptc */

namespace {

/* the shutter of a wpt_render_shutter_* call as the launch carries it, checked against the frame's rows and the exposure interval */
wpt_status shutterOfCall(const wpt_shutter* shutter, const wpt_params* params, uint32_t height, wptshutter::Rows& rows)
{
    if (!shutter || !params)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* why = wptshutter::refusal(shutter->row_time, shutter->from_top, shutter->reserved[0], shutter->reserved[1], params->t0, params->t1, height))
        return fail(WPT_ERR_INVALID_ARGUMENT, why);
    rows = { shutter->row_time, shutter->from_top };
    return WPT_OK;
}

/* a block of consecutive pixels; shutter: NULL for wpt_render_block_device */
wpt_status blockDevice(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame_device, hip_stream };
    rq.counters = counters_device;
    if (shutter)
        WPT_TRY(shutterOfCall(shutter, params, height, rq.shutter));
    return renderLaunch(rq);
}

/* one rank's interleaved bands in one launch; shutter: NULL for wpt_render_bands_device */
wpt_status bandsDevice(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    if (band_rows == 0 || band_stride == 0 || first_band >= band_stride || width == 0 || height == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands need band_rows > 0 and first_band < band_stride");
    const uint64_t bandPixels = uint64_t(band_rows) * width;
    const uint64_t bands = (uint64_t(height) + band_rows - 1) / band_rows;
    const uint64_t mine = first_band < bands ? (bands - first_band + band_stride - 1) / band_stride : 0;
    if (bandPixels > 0xffffffffull || mine * bandPixels > 0xffffffffull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands too large");
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, 0, uint32_t(mine * bandPixels), frame_device, hip_stream };
    rq.bandPixels = uint32_t(bandPixels);
    rq.bandFirst = first_band;
    rq.bandStride = band_stride;
    rq.counters = counters_device;
    if (shutter)
        WPT_TRY(shutterOfCall(shutter, params, height, rq.shutter));
    return renderLaunch(rq);
}

/* ... and their synchronous forms for host memory */
wpt_status bandsHost(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host)
{
    if (!frame_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "frame_host is NULL");
    if (width == 0 || height == 0 || band_rows == 0 || band_stride == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands need a frame, band_rows > 0 and band_stride > 0");
    wptshutter::Rows checked;
    if (shutter) /* (refused before any memory is asked for) */
        WPT_TRY(shutterOfCall(shutter, params, height, checked));
    StagedBlock frame;
    const size_t rowBytes = size_t(width) * 3 * sizeof(float);
    HIP_TRY(frame.allocate(rowBytes * height));
    WPT_TRY(bandsDevice(scene, camera, params, shutter, width, height, samples_sqrt, band_rows, first_band, band_stride,
            static_cast<float*>(frame.device), nullptr, nullptr));
    WPT_TRY(wpt_scene_check(scene));
    for (uint64_t band = first_band; band * band_rows < height; band += band_stride) {
        const size_t row0 = size_t(band) * band_rows;
        const size_t rows = row0 + band_rows <= height ? band_rows : height - row0;
        WPT_TRY(hipStatus("hipMemcpy", hipMemcpy(reinterpret_cast<char*>(frame_host) + row0 * rowBytes, static_cast<char*>(frame.device) + row0 * rowBytes,
                rows * rowBytes, hipMemcpyDeviceToHost)));
    }
    return WPT_OK;
}

wpt_status blockHost(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter, uint32_t width,
        uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb)
{
    if (!block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_rgb is NULL");
    wptshutter::Rows checked;
    if (shutter) /* (refused before any memory is asked for, and for an empty block too) */
        WPT_TRY(shutterOfCall(shutter, params, height, checked));
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block;
    HIP_TRY(block.allocatePixels(block_size));
    return finishStaged(blockDevice(scene, camera, params, shutter, width, height, samples_sqrt, block_start, block_size,
            block.biased(block_start), nullptr, nullptr), scene, block, block_rgb);
}

const char* const NULL_SHUTTER = "shutter is NULL";

} /* namespace */

extern "C" {

wpt_status wpt_render_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    return blockDevice(scene, camera, params, nullptr, width, height, samples_sqrt, block_start, block_size, frame_device, counters_device, hip_stream);
}

wpt_status wpt_render_bands_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    return bandsDevice(scene, camera, params, nullptr, width, height, samples_sqrt, band_rows, first_band, band_stride, frame_device, counters_device,
            hip_stream);
}

wpt_status wpt_render_bands(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host)
{
    return bandsHost(scene, camera, params, nullptr, width, height, samples_sqrt, band_rows, first_band, band_stride, frame_host);
}

wpt_status wpt_render_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width,
        uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb)
{
    return blockHost(scene, camera, params, nullptr, width, height, samples_sqrt, block_start, block_size, block_rgb);
}

/* ---- the rolling shutter: the same launches with a row's interval in the place of [t0, t1] (wpt_shutter.h) ---- */

wpt_status wpt_shutter_row_interval(const wpt_shutter* shutter, float t0, float t1, uint32_t height, uint32_t row, float* a, float* b)
{
    if (!shutter || !a || !b)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* why = wptshutter::refusal(shutter->row_time, shutter->from_top, shutter->reserved[0], shutter->reserved[1], t0, t1, height))
        return fail(WPT_ERR_INVALID_ARGUMENT, why);
    if (row >= height)
        return fail(WPT_ERR_INVALID_ARGUMENT, "shutter: row lies outside the frame");
    const wptshutter::Interval iv = wptshutter::rowInterval({ shutter->row_time, shutter->from_top }, t0, t1, height, row);
    *a = iv.a;
    *b = iv.b;
    return WPT_OK;
}

wpt_status wpt_shutter_span(const wpt_shutter* shutter, float t0, float t1, uint32_t height, float* first, float* last)
{
    if (!shutter || !first || !last)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* why = wptshutter::refusal(shutter->row_time, shutter->from_top, shutter->reserved[0], shutter->reserved[1], t0, t1, height))
        return fail(WPT_ERR_INVALID_ARGUMENT, why);
    /* the row read first opens at t0, the row read last closes at b(k = height - 1), whichever end of the frame that is */
    *first = t0;
    *last = wptshutter::rowInterval({ shutter->row_time, 0u }, t0, t1, height, height - 1u).b;
    return WPT_OK;
}

wpt_status wpt_render_shutter_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    if (!shutter)
        return fail(WPT_ERR_INVALID_ARGUMENT, NULL_SHUTTER);
    return blockDevice(scene, camera, params, shutter, width, height, samples_sqrt, block_start, block_size, frame_device, counters_device, hip_stream);
}

wpt_status wpt_render_shutter_bands_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    if (!shutter)
        return fail(WPT_ERR_INVALID_ARGUMENT, NULL_SHUTTER);
    return bandsDevice(scene, camera, params, shutter, width, height, samples_sqrt, band_rows, first_band, band_stride, frame_device, counters_device,
            hip_stream);
}

wpt_status wpt_render_shutter_bands(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host)
{
    if (!shutter)
        return fail(WPT_ERR_INVALID_ARGUMENT, NULL_SHUTTER);
    return bandsHost(scene, camera, params, shutter, width, height, samples_sqrt, band_rows, first_band, band_stride, frame_host);
}

wpt_status wpt_render_shutter_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb)
{
    if (!shutter)
        return fail(WPT_ERR_INVALID_ARGUMENT, NULL_SHUTTER);
    return blockHost(scene, camera, params, shutter, width, height, samples_sqrt, block_start, block_size, block_rgb);
}

} /* extern "C" */
