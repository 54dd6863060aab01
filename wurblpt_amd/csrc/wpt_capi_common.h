/*
 * wpt_capi_common.h -- what the units behind include/wurblpt_hip.h (wpt_capi*.hip) share, and nothing that only one of them
 * uses.  All of it is in namespace wptc, whose visibility is hidden: the library exports the C ABI and nothing of this.  The
 * output side (wpt_capi_postproc.hip) defines WPT_CAPI_OUTPUT_SIDE and sees the first part only, which needs no header of the
 * path tracer.
 */
#ifndef WPT_CAPI_COMMON_H
#define WPT_CAPI_COMMON_H

#include <hip/hip_runtime.h>

#include <cassert>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wurblpt_hip.h"
#ifndef WPT_CAPI_OUTPUT_SIDE
#include "wpt_kernel_table.h"
#include "wpt_launch_plan.h"
#include "wpt_wavefront.inc.h"
#include "wpt_bypass.h"
#endif

namespace wptc __attribute__((visibility("hidden"))) {

/* sets the calling thread's message, which wpt_last_error reads (one object for the library, in wpt_capi.hip), and returns s */
wpt_status fail(wpt_status s, const std::string& msg);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(WPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)
#define WPT_TRY(expr)                                                                              \
    do {                                                                                           \
        const wpt_status s_ = (expr);                                                              \
        if (s_ != WPT_OK)                                                                          \
            return s_;                                                                             \
    } while (0)

/* WPT_OK, or "<what>: <HIP's text for e>" as WPT_ERR_HIP -- as WPT_ERR_OUT_OF_MEMORY where oomToo is set and e says so */
inline wpt_status hipStatus(const char* what, hipError_t e, bool oomToo = false)
{
    if (e == hipSuccess)
        return WPT_OK;
    return fail(oomToo && e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

/* do the byte ranges [a, a + bytesA) and [b, b + bytesB) share a byte? */
inline bool overlaps(const void* a, size_t bytesA, const void* b, size_t bytesB)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytesB && y < x + bytesA;
}

/* The stream-ordered scratch memory of one launch (the pool's counter, carry, cost, order, work words, slice words and carry; a
 * sensor's table, a batch's cameras, a denoiser's records): launches in flight on any number of streams never share any of it;
 * freed in stream order when the owner goes out of scope, behind the read of the launch's error. */
struct StreamScratch {
    hipStream_t stream;
    void* held[5] = {}; /* the counter and the four arrays of two passes: no launch asks for more */
    uint32_t count = 0;
    explicit StreamScratch(hipStream_t s) : stream(s) {}
    StreamScratch(const StreamScratch&) = delete;
    ~StreamScratch()
    {
        for (uint32_t i = 0; i < count; i++)
            (void)hipFreeAsync(held[i], stream);
    }
    /* n elements at *p, or the error for the caller to report */
    template<typename T> hipError_t get(size_t n, T** p)
    {
        assert(count < sizeof(held) / sizeof(held[0]));
        const hipError_t e = hipMallocAsync(reinterpret_cast<void**>(p), n * sizeof(T), stream);
        if (e == hipSuccess)
            held[count++] = *p;
        return e;
    }
    /* n elements, or NULL where the memory cannot be had: the error is cleared, the launch goes without */
    template<typename T> T* get(size_t n)
    {
        T* p = nullptr;
        if (get(n, &p) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return p;
    }
};

#ifndef WPT_CAPI_OUTPUT_SIDE

} /* namespace wptc */

struct wpt_scene {
    int device;
    wptd::SceneView view;
    uint32_t features;
    uint32_t nodeCount, triCount;
    uint32_t foldedLinks; /* wpt_scene_folded_links */
    /* a scene that fits LDS: the link words of its tree's copy there (wpt_bypass.h, Plan), three arrays of 2 * nodeCount + 4
     * words one behind the other -- plain, folded, bypass -- and the inner nodes the last one leaves out; else NULL */
    uint32_t* ldsLinks = nullptr;
    /* ... and behind them the same three sets for the kernels with rotated corner copies (wpt_leaf_words.h: leaf words that say
     * where the corners lie, and per triangle its leaf's skip link), wptw::leafWordsSize words each.  leafOneToOne: every
     * triangle has exactly one leaf, so the leaf pass of those kernels takes its links from the corner records */
    bool leafOneToOne = false;
    /* ... and, where every box of the tree has lo <= hi (no NaN bound either), the node array once per sign octant of a ray's
     * direction for the kernels of 1024 lanes (wpt_scene_layout.h, orderedBoxCopies); else NULL */
    const float4* orderedNodes = nullptr;
    /* the instances whose normal matrix a triangle with WPT_TRI_TRANSFORM names: 0 .. normalsNamed - 1 (0: no triangle is
     * transformed), which the kernels of 1024 lanes keep in LDS where there is room (wpt_lds_places.h) */
    uint32_t normalsNamed = 0;
    uint32_t bypassedNodes = 0; /* wpt_scene_bypassed_nodes */
    uint32_t animationCount;
    std::vector<void*> allocations;
    int cuCount;
    std::vector<float> envM, envMcs;
    std::vector<int32_t> envMs;
};

namespace wptc __attribute__((visibility("hidden"))) {

/* The process's settings (wpt_set_*), one instance, defined in wpt_capi.hip.  Launches and uploads read them without a lock, as
 * they always have: a caller sets them before its threads render. */
struct Settings {
    uint32_t threadsPerGroup = wptk::WG;
    uint32_t variant = 0;
    uint32_t leaveEighths = 0; /* 0 = default: chosen per scene size (single-role kernel) / patience 8 rounds (ray-pool kernel) */
    uint32_t heavyMin = 0; /* 0 = chosen per scene size at launch */
    uint32_t leafBias = 0;
    uint32_t topNodes = 65536; /* nodes of a large tree that are stored level by level in front (wpt_set_top_nodes) */
    unsigned long long* schedStats = nullptr;
    /* wpt_set_wavefront: 0 = the library decides, 1 = wavefront wherever it exists, 2 = never; launch geometry (0 = defaults) */
    uint32_t wfMode = 0;
    wptk::WfConfig wfConfig = { 0, 0, 0, 1, 0, 0, 0, 0, 0 };
    /* wpt_set_walk: WPT_WALK_* bits */
    uint32_t walk = 0;
    /* wpt_set_bypass: how scenes uploaded from now on choose the nodes their walk leaves out (wpt_bypass.h) */
    uint32_t bypassMode = wptb::MODE_MODEL;
    /* wpt_set_slices: 0 = wpt_slices_plan, 1 = never, 2 .. 15 = that many units; WPT_SLICES_DECLINE_ODD beside it */
    uint32_t slices = 0;
};
extern Settings settings;

/* what the process's most recent render call ran (wpt_capi.hip has the words and their readers), the form's name and the
 * kernel table's row of an instantiation: see their definitions there */
void recordLaunch(const char* name, const char* form, uint32_t passes, unsigned long long* sliceStats);
void recordWorkgroup(uint32_t lanes, bool orderedBoxes, uint32_t hitDataParts, bool materialsByLdsAddress, bool launchRecord);
const char* kernelForm(bool rotated, uint32_t units = 0, bool leafLinksFromNodes = false);
wpt_status lookupKernel(uint32_t features, bool count, bool ldsScene, bool wide, const wptk::KernelEntry** entry);

/* One launch of the path tracer: a block of consecutive pixels (bandStride == 0) or interleaved bands of bandPixels pixels, and
 * the one sensor it renders for, whose view is the member that `sensor` names.  Every caller sets the first ten members. */
struct LaunchRequest {
    wpt_scene* scene;
    const wpt_camera* camera; /* SENSOR_VIEWS: the first of views.viewCount host cameras, the block all their pixels */
    const wpt_params* params;
    uint32_t width, height, samplesSqrt, blockStart, blockSize;
    float* frame; /* may be NULL for the transient film and for several time-of-flight phases */
    void* stream;
    wpt_counters* counters = nullptr;
    uint32_t bandPixels = 0, bandFirst = 0, bandStride = 0;
    wptk::Sensor sensor = wptk::SENSOR_FRAME;
    wptk::BinsView bins = {};         /* SENSOR_TRANSIENT, SENSOR_TOF (wpt_blocks.h, accumulate) */
    wptk::ViewsView views = {};       /* SENSOR_VIEWS */
    wptk::AdaptiveView adaptive = {}; /* SENSOR_ADAPTIVE */
    wptshutter::Rows shutter = { 0.0f, 0u }; /* SENSOR_FRAME: the rolling shutter, checked by the caller (wpt_render_shutter_*); zeros: none */
};

/* the launch itself and its parts, which a session's stage is made of too (wpt_capi_render.hip) */
wpt_status checkFrameBlock(uint32_t width, uint32_t height, const uint32_t* samplesSqrt, uint32_t blockStart, uint32_t blockSize,
        uint32_t frames = 1, const char* prefix = "", bool session = false);
wpt_status launchSetUp(const wpt_scene* scene, const wpt_camera* camera, uint32_t cameraCount, bool batch, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        uint32_t band_pixels, uint32_t band_first, uint32_t band_stride, bool count, wptk::KernelArgs& args, uint32_t& need);
hipError_t runSingleKernel(const wpt_scene* scene, wptk::KernelArgs& args, const wptk::KernelChoice& choice, const wptk::KernelEntry* kernel,
        const wptk::KernelEntry* slicedTwin, const wptk::LaunchPlan& plan, hipStream_t stream);
wpt_status renderLaunch(const LaunchRequest& rq);

/* the work words of the order kernels (wpt_k_order.hip); the last is the number of entries of the order they build */
constexpr size_t ORDER_WORK_WORDS = 3 * wptk::ORDER_BUCKETS + 1;

/* `order` from the costs `measured` left per pixel, the costliest 8x8 tiles first, for `next` to take its pixels in */
inline void orderByCost(const wptk::KernelArgs& measured, uint32_t* order, uint32_t* work, hipStream_t stream, wptk::KernelArgs& next)
{
    wptk::launchOrderBuild(measured, order, work, stream);
    next.order = order;
    next.orderCount = work + ORDER_WORK_WORDS - 1;
}

/* Device memory of a host entry point for a block's pixels only, not a frame's: the launch gets a pointer biased so that pixel
 * `blockStart` lands at offset 0.  Freed at scope exit. */
struct StagedBlock {
    void* device = nullptr;
    size_t bytes = 0;
    StagedBlock() = default;
    StagedBlock(const StagedBlock&) = delete;
    ~StagedBlock() { (void)hipFree(device); }
    hipError_t allocate(size_t n) { return hipMalloc(&device, bytes = n); }
    hipError_t allocatePixels(size_t pixels, size_t planes = 1) { return allocate(pixels * 3 * sizeof(float) * planes); }
    hipError_t upload(const void* host) { return hipMemcpy(device, host, bytes, hipMemcpyHostToDevice); }
    hipError_t download(void* host) const { return device ? hipMemcpy(host, device, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    /* NULL without memory: an output the caller did not ask for */
    float* biased(uint32_t blockStart) const { return device ? static_cast<float*>(device) - size_t(blockStart) * 3 : nullptr; }
};

/* The end of a host entry point: behind a launch that went well, waits for the device and reports what its kernels ran into
 * (wpt_scene_check; check == NULL: the launch is not the scene's), then copies the staged blocks that exist to their host arrays. */
inline wpt_status finishStaged(wpt_status launched, wpt_scene* check, const StagedBlock& a, void* hostA, const StagedBlock* b = nullptr, void* hostB = nullptr)
{
    const wpt_status st = launched == WPT_OK && check ? wpt_scene_check(check) : launched;
    hipError_t e = st == WPT_OK ? a.download(hostA) : hipSuccess;
    if (st == WPT_OK && e == hipSuccess && b)
        e = b->download(hostB);
    return e == hipSuccess ? st : hipStatus("hipMemcpy", e);
}

#endif /* WPT_CAPI_OUTPUT_SIDE */

} /* namespace wptc */

#endif
