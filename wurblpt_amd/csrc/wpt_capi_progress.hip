/*
 * wpt_capi_progress.hip -- of include/wurblpt_hip.h: a frame in resumable stages, struct wpt_progress and every wpt_progress_*.
 * A stage is the launch of wpt_capi_render.hip with the strategy fixed by the session; what a saved state holds is
 * wpt_progress_state.h, the session's own small kernels are wpt_k_progress.hip.
 */
#include <cstring>

#include "wpt_capi_common.h"
#include "wpt_progress.h"
#include "wpt_progress_state.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

struct wpt_progress {
    wpt_scene* scene;
    wptk::KernelArgs args; /* of the one-shot launch of the block; a stage sets frame, rowStop, order, orderCount and pool */
    wptk::KernelChoice choice;
    const wptk::KernelEntry* kernel;
    uint32_t rowsDone;
    uint64_t tag;
    /* device memory for the session's lifetime: carry and cost per pixel of the frame (the kernels index them by the frame's
     * pixel), order per pixel of the block, the order kernels' work words */
    float4* carry;
    uint32_t *cost, *order, *work;
    bool frameOrderBuilt; /* scene in LDS: `order` holds the frame's own order, which every later stage takes */
    hipStream_t lastStream;
};

namespace {

void progressFree(wpt_progress* p)
{
    for (void* m : { static_cast<void*>(p->carry), static_cast<void*>(p->cost), static_cast<void*>(p->order), static_cast<void*>(p->work) })
        if (m)
            (void)hipFree(m);
    delete p;
}

wpt_progress_info progressInfo(const wpt_progress* p)
{
    wpt_progress_info i;
    memset(&i, 0, sizeof(i));
    i.version = WPT_PROGRESS_STATE_VERSION;
    i.width = p->args.width;
    i.height = p->args.height;
    i.samples_sqrt = p->args.samplesSqrt;
    i.block_start = p->args.blockStart;
    i.block_size = p->args.blockSize;
    i.rows_done = p->rowsDone;
    i.tag = p->tag;
    i.state_bytes = uint64_t(wptp::STATE_HEADER_BYTES) + uint64_t(i.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL;
    return i;
}

} /* namespace */

extern "C" {

wpt_status wpt_progress_covers(uint32_t sensor, uint32_t counting, uint32_t bands)
{
    static const char* const sensors[] = { nullptr, "the transient film", "a batch of views", "an adaptive map", "the time-of-flight sensor" };
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor must lie in 0 .. 4");
    if (sensors[sensor])
        return fail(WPT_ERR_UNSUPPORTED, std::string("sessions render one frame, not ") + sensors[sensor]
                + ": what a pixel carries between stages is its generator and three sums");
    if (counting)
        return fail(WPT_ERR_UNSUPPORTED, "sessions do not cover counting launches: the counters of a stage would count the launch's lanes, not the rows rendered");
    if (bands)
        return fail(WPT_ERR_UNSUPPORTED, "sessions do not cover bands: a session renders one block of consecutive pixels");
    return WPT_OK;
}

wpt_status wpt_progress_begin(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, uint64_t tag, wpt_progress** out_progress)
{
    if (out_progress)
        *out_progress = nullptr;
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; the path tracer has no CPU fallback");
    if (!scene || !camera || !params || !out_progress)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(checkFrameBlock(width, height, &samples_sqrt, block_start, block_size, 1, "", true));
    /* the arguments and the kernel of the plain frame launch without counters, set up by what renderLaunch sets them up with */
    wpt_progress* p = new wpt_progress{}; /* (zeros: no row done, no memory yet, the null stream) */
    p->scene = scene;
    p->tag = tag;
    KernelArgs& args = p->args;
    uint32_t need = 0;
    const wpt_status setUp = launchSetUp(scene, camera, 1, false, params, width, height, samples_sqrt, block_start, block_size, 0, 0, 0, false, args, need);
    if (setUp != WPT_OK) {
        progressFree(p);
        return setUp;
    }
    args.bins = wptk::BinsView{};
    p->choice = wptk::selectKernel({ need, wptk::SENSOR_FRAME, false, scene->nodeCount, scene->triCount, uint32_t(scene->view.materialCount),
            scene->view.wideNodes != nullptr, settings.variant, settings.walk });
    const wpt_status found = lookupKernel(p->choice.features, p->choice.count, p->choice.ldsScene, p->choice.wide, &p->kernel);
    if (found != WPT_OK) {
        progressFree(p);
        return found;
    }
    args.materialsInLds = p->choice.materialsInLds;
    /* hipMalloc, not stream-ordered: the memory outlives the calls.  Carry and cost start as zeros: a state saved before the
     * first stage is defined, and so is the order that a restored session builds from times it never measured. */
    const size_t pixels = size_t(width) * height;
    const size_t workBytes = ORDER_WORK_WORDS * sizeof(uint32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->carry), pixels * 2 * sizeof(float4));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->cost), pixels * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->order), size_t(block_size) * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->work), workBytes);
    if (e == hipSuccess)
        e = hipMemset(p->carry + 2 * size_t(block_start), 0, size_t(block_size) * 2 * sizeof(float4));
    if (e == hipSuccess)
        e = hipMemset(p->cost, 0, pixels * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        progressFree(p);
        return hipStatus("session memory (40 bytes per pixel)", e, true);
    }
    args.carry = p->carry;
    args.cost = p->cost;
    *out_progress = p;
    return WPT_OK;
}

wpt_status wpt_progress_advance_device(wpt_progress* p, uint32_t rows, float* frame_device, void* hip_stream)
{
    if (!p)
        return fail(WPT_ERR_INVALID_ARGUMENT, "progress is NULL");
    const uint32_t total = p->args.samplesSqrt;
    if (rows == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "a stage renders at least one row of strata: rows is 0");
    if (p->rowsDone >= total)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the session is finished: all " + std::to_string(total) + " rows of strata are rendered");
    const uint32_t rowStop = rows < total - p->rowsDone ? p->rowsDone + rows : total;
    if (rowStop == total && !frame_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the stage that finishes the frame needs frame_device: it is NULL");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    wptk::KernelArgs stage = p->args;
    stage.frame = frame_device;
    stage.rowStop = rowStop;
    stage.schedStats = nullptr;
    if (p->rowsDone > 0 && !p->choice.sceneInLds) {
        /* a stage that resumes takes its pixels from `order` and loads what they carry: for the scene in HBM the tiles that
         * took the stage before longest first, as the second of the one-shot launch's two passes does */
        orderByCost(p->args, p->order, p->work, stream, stage);
    } else if (p->rowsDone > 0) {
        /* ... and the frame's own order for the scene in LDS (any other costs those kernels more than it gains) */
        if (!p->frameOrderBuilt)
            wptk::launchProgressFrameOrder(p->args, p->order, p->work + ORDER_WORK_WORDS - 1, stream);
        p->frameOrderBuilt = true;
        stage.order = p->order;
        stage.orderCount = p->work + ORDER_WORK_WORDS - 1;
    }
    /* planned as a frame launch without counters (with the variant word of this moment) whose strategy the session has fixed:
     * one pass, in the order set up above */
    const bool pooled = wptk::planLaunch({ wptk::SENSOR_FRAME, false, false, false, p->choice.sceneInLds, stage.blockSize, total, stage.cuCount,
            settings.variant, 2u, 1u }).pooled;
    HIP_TRY(runSingleKernel(p->scene, stage, p->choice, p->kernel, nullptr, { false, false, pooled, wptk::ONE_PASS, 1, total, 1 }, stream));
    /* The launch that renders the last row writes the frame and stores no carry.  A finished session keeps the block's pixels
     * of its frame in the carry's place instead, so that its preview and its saved state still yield the frame. */
    if (rowStop == total) {
        wptk::launchProgressCapture(frame_device, p->carry, p->args.blockStart, p->args.blockSize, total << 16, stream);
        HIP_TRY(hipGetLastError());
    }
    p->rowsDone = rowStop;
    p->lastStream = stream;
    return WPT_OK;
}

wpt_status wpt_progress_advance(wpt_progress* p, uint32_t rows, float* block_rgb)
{
    if (!p)
        return fail(WPT_ERR_INVALID_ARGUMENT, "progress is NULL");
    const uint32_t total = p->args.samplesSqrt;
    const bool finishes = rows > 0 && p->rowsDone < total && rows >= total - p->rowsDone;
    if (finishes && !block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the stage that finishes the frame needs block_rgb: it is NULL");
    StagedBlock block;
    if (finishes)
        HIP_TRY(block.allocatePixels(p->args.blockSize));
    return finishStaged(wpt_progress_advance_device(p, rows, block.biased(p->args.blockStart), nullptr), p->scene, block, block_rgb);
}

uint32_t wpt_progress_rows_done(const wpt_progress* p)
{
    return p ? p->rowsDone : 0u;
}

uint32_t wpt_progress_rows_total(const wpt_progress* p)
{
    return p ? p->args.samplesSqrt : 0u;
}

wpt_status wpt_progress_preview_device(wpt_progress* p, float* frame_device, void* hip_stream)
{
    if (!p || !frame_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* (a finished session's carry holds the pixels' values themselves, and a session without a stage zeros) */
    const uint32_t total = p->args.samplesSqrt;
    const float inv = p->rowsDone == total ? 1.0f : (p->rowsDone ? 1.0f / float(p->rowsDone * total) : 0.0f);
    wptk::launchProgressResolve(p->carry, frame_device, p->args.blockStart, p->args.blockSize, inv, stream);
    HIP_TRY(hipGetLastError());
    p->lastStream = stream;
    return WPT_OK;
}

wpt_status wpt_progress_preview(wpt_progress* p, float* block_rgb)
{
    if (!p || !block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock block;
    HIP_TRY(hipStreamSynchronize(p->lastStream));
    HIP_TRY(block.allocatePixels(p->args.blockSize));
    return finishStaged(wpt_progress_preview_device(p, block.biased(p->args.blockStart), nullptr), nullptr, block, block_rgb);
}

void wpt_progress_end(wpt_progress* p)
{
    if (!p)
        return;
    (void)hipStreamSynchronize(p->lastStream);
    progressFree(p);
}

wpt_status wpt_progress_state_bytes(const wpt_progress* p, uint64_t* bytes)
{
    if (!p || !bytes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *bytes = progressInfo(p).state_bytes;
    return WPT_OK;
}

wpt_status wpt_progress_save(wpt_progress* p, void* buffer_host, uint64_t bytes)
{
    if (!p || !buffer_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const wpt_progress_info info = progressInfo(p);
    if (bytes != info.state_bytes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the buffer must hold wpt_progress_state_bytes = " + std::to_string(info.state_bytes) + " bytes, not "
                + std::to_string(bytes));
    HIP_TRY(hipStreamSynchronize(p->lastStream));
    wptp::writeStateHeader(buffer_host, info, p->args.cam, p->args.par);
    HIP_TRY(hipMemcpy(static_cast<unsigned char*>(buffer_host) + wptp::STATE_HEADER_BYTES, p->carry + 2 * size_t(info.block_start),
            size_t(info.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL, hipMemcpyDeviceToHost));
    return WPT_OK;
}

wpt_status wpt_progress_state_info(const void* buffer_host, uint64_t bytes, wpt_progress_info* info)
{
    if (!info)
        return fail(WPT_ERR_INVALID_ARGUMENT, "info is NULL");
    if (bytes > uint64_t(SIZE_MAX))
        return fail(WPT_ERR_INVALID_ARGUMENT, "the state is longer than its header says");
    const char* refused = wptp::parseState(buffer_host, size_t(bytes), info);
    return refused ? fail(WPT_ERR_INVALID_ARGUMENT, refused) : WPT_OK;
}

wpt_status wpt_progress_restore(wpt_scene* scene, const void* buffer_host, uint64_t bytes, const wpt_camera* camera, const wpt_params* params,
        uint64_t tag, wpt_progress** out_progress)
{
    if (out_progress)
        *out_progress = nullptr;
    if (!scene || !camera || !params || !out_progress)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    wpt_progress_info info;
    const wpt_status parsed = wpt_progress_state_info(buffer_host, bytes, &info);
    if (parsed != WPT_OK)
        return parsed;
    const unsigned char* state = static_cast<const unsigned char*>(buffer_host);
    const char* differs = info.tag != tag ? "tag" : memcmp(state + wptp::STATE_CAMERA, camera, sizeof(*camera)) != 0 ? "camera"
            : memcmp(state + wptp::STATE_PARAMS, params, sizeof(*params)) != 0 ? "params" : nullptr;
    if (differs)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string("the state was saved with a different ") + differs);
    /* the body, as far as the header says what it holds: every pixel stands at the first stratum of row rows_done */
    const uint64_t damaged = wptp::firstDamagedRecord(state, info);
    if (damaged < info.block_size)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the state is damaged: the record of pixel " + std::to_string(uint64_t(info.block_start) + damaged)
                + " does not stand at row rows_done of its strata");
    wpt_progress* p = nullptr;
    const wpt_status begun = wpt_progress_begin(scene, camera, params, info.width, info.height, info.samples_sqrt, info.block_start, info.block_size,
            tag, &p);
    if (begun != WPT_OK)
        return begun;
    const hipError_t e = hipMemcpy(p->carry + 2 * size_t(info.block_start), state + wptp::STATE_HEADER_BYTES,
            size_t(info.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        progressFree(p);
        return hipStatus("hipMemcpy", e);
    }
    p->rowsDone = info.rows_done;
    *out_progress = p;
    return WPT_OK;
}

} /* extern "C" */
