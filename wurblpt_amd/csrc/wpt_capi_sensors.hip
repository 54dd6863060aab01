/*
 * wpt_capi_sensors.hip -- of include/wurblpt_hip.h: the sensors beside the plain frame, each a request to the launch of
 * wpt_capi_render.hip: the transient film, light groups, the time-of-flight sensor (with wpt_tof_accumulate_host), batches of
 * views, view streams and the split render, and adaptive sampling.  Each sensor's checks stand above its entry points.
 */
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "wpt_capi_common.h"
#include "wpt_lightmix.h"
#include "wpt_streams_launch.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

namespace {

/* the transient film's planes after the launch: plane value = 1 / samples * accumulated value (SensorRGB::finishPixel) for the
 * block's pixels of every plane */
__global__ void wpt_transient_finish_kernel(float* bins, size_t stride, uint32_t blockStart, uint32_t blockSize, uint32_t binCount, float invSamples)
{
    const uint64_t perPlane = uint64_t(blockSize) * 3, n = perPlane * binCount;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        float* p = bins + (i / perPlane) * stride + size_t(blockStart) * 3 + i % perPlane;
        *p = invSamples * *p;
    }
}

} /* namespace */

extern "C" {

/* One launch into planes of accumulated values, the transient film's or the time-of-flight sensor's.  `table`, the sensor's
 * words, goes to the device as rq.bins.edges; where the kernels accumulate into the planes (`accumulated`), the planes' block is
 * zeroed before the render and scaled by 1 / samples behind it, all in stream order.  rq.bins.bins is plane 0's pixel 0 with
 * rq.bins.stride floats between planes (a full frame's, or a block's behind a biased pointer); what: the sensor, for messages. */
static wpt_status planesLaunch(LaunchRequest rq, const float* table, size_t tableFloats, bool accumulated, const char* what)
{
    const wptk::BinsView& bv = rq.bins;
    hipStream_t stream = static_cast<hipStream_t>(rq.stream);
    StreamScratch scratch(stream);
    float* dTable = nullptr;
    WPT_TRY(hipStatus(what, scratch.get(tableFloats, &dTable)));
    hipError_t e = hipMemcpyAsync(dTable, table, tableFloats * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && accumulated)
        e = hipMemset2DAsync(bv.bins + size_t(rq.blockStart) * 3, bv.stride * sizeof(float), 0, size_t(rq.blockSize) * 3 * sizeof(float), bv.binCount,
                stream);
    WPT_TRY(hipStatus(what, e));
    rq.bins.edges = dTable;
    WPT_TRY(renderLaunch(rq));
    if (accumulated) {
        const uint64_t n = uint64_t(rq.blockSize) * 3 * bv.binCount;
        const uint32_t blocks = uint32_t(std::min<uint64_t>((n + 255) / 256, 65536));
        hipLaunchKernelGGL(wpt_transient_finish_kernel, dim3(blocks), dim3(256), 0, stream, bv.bins, bv.stride, rq.blockStart, rq.blockSize,
                bv.binCount, 1.0f / float(rq.samplesSqrt * rq.samplesSqrt));
        e = hipGetLastError();
    }
    return hipStatus(what, e);
}

/* refuses a bad edge set; fills what the kernels need of a good one but the device copy of the edges */
static wpt_status transientEdges(const float* edges, uint32_t binCount, wptk::BinsView& bv)
{
    if (!edges)
        return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edges are NULL");
    if (binCount == 0 || binCount > WPT_TRANSIENT_MAX_BINS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin count must lie in 1 .. " + std::to_string(WPT_TRANSIENT_MAX_BINS));
    for (uint32_t k = 0; k <= binCount; k++) {
        if (std::isnan(edges[k]))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edge " + std::to_string(k) + " is NaN");
        if (std::isinf(edges[k]) && !(k == binCount && edges[k] > 0.0f))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edge " + std::to_string(k) + " is infinite (only the last may be +inf)");
        if (k > 0 && !(edges[k] > edges[k - 1]))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edges must increase (edge " + std::to_string(k) + ")");
    }
    /* the kernels' first guess of a bin: uniform spacing between the first and the last finite edge */
    const uint32_t lastFinite = std::isinf(edges[binCount]) ? binCount - 1 : binCount;
    float scale = lastFinite > 0 ? float(lastFinite) / (edges[lastFinite] - edges[0]) : 0.0f;
    bv = wptk::BinsView{};
    bv.binCount = binCount;
    bv.guessScale = std::isfinite(scale) ? scale : 0.0f;
    return WPT_OK;
}

/* one transient launch; `bins` and `stride` as planesLaunch takes them */
static wpt_status transientLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const float* edges, uint32_t binCount,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* frame, float* bins,
        size_t stride, hipStream_t stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame, stream };
    WPT_TRY(transientEdges(edges, binCount, rq.bins));
    if (!scene || !camera || !params || !bins)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    rq.sensor = wptk::SENSOR_TRANSIENT;
    rq.bins.bins = bins;
    rq.bins.stride = stride;
    rq.bins.width = width;
    return planesLaunch(rq, edges, size_t(binCount) + 1, true, "transient film");
}

wpt_status wpt_render_transient_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const float* edges_host, uint32_t bin_count, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start,
        uint32_t block_size, float* frame_device, float* bins_device, void* hip_stream)
{
    return transientLaunch(scene, camera, params, edges_host, bin_count, width, height, samples_sqrt, block_start, block_size,
            frame_device, bins_device, size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_transient_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const float* edges_host, uint32_t bin_count, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start,
        uint32_t block_size, float* block_rgb, float* block_bins)
{
    wptk::BinsView bv;
    WPT_TRY(transientEdges(edges_host, bin_count, bv));
    if (!block_bins)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_bins is NULL");
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block, bins;
    if (block_rgb)
        HIP_TRY(block.allocatePixels(block_size));
    const hipError_t e = bins.allocatePixels(block_size, bin_count);
    if (e != hipSuccess)
        return fail(WPT_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    return finishStaged(transientLaunch(scene, camera, params, edges_host, bin_count, width, height, samples_sqrt, block_start, block_size,
            block.biased(block_start), bins.biased(block_start), size_t(block_size) * 3, nullptr), scene, block, block_rgb, &bins, block_bins);
}

/* refuses a bad light-groups table; fills what the kernels need of a good one but the device copy of the table */
static wpt_status lightGroupsTable(const uint8_t* groupOfMaterial, uint32_t materialCount, uint32_t groupCount, uint32_t envGroup, wptk::BinsView& bv)
{
    uint32_t at = 0;
    switch (wptmix::checkTable(groupOfMaterial, materialCount, groupCount, envGroup, &at)) {
    case wptmix::TABLE_OK:
        break;
    case wptmix::TABLE_NULL:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the table of the materials' groups is NULL");
    case wptmix::TABLE_GROUP_COUNT:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: group count must lie in 1 .. " + std::to_string(WPT_LIGHT_GROUPS_MAX));
    case wptmix::TABLE_ENTRY:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: material " + std::to_string(at) + " has group " + std::to_string(groupOfMaterial[at])
                + ", which is neither below the group count " + std::to_string(groupCount) + " nor WPT_LIGHT_GROUP_NONE");
    case wptmix::TABLE_ENV_GROUP:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the environment's group " + std::to_string(envGroup)
                + " is neither below the group count " + std::to_string(groupCount) + " nor WPT_LIGHT_GROUP_NONE");
    }
    bv = wptk::BinsView{};
    bv.binCount = groupCount;
    bv.rule = wptk::BINS_BY_EMITTER | envGroup;
    return WPT_OK;
}

/* one light-groups launch: a launch of the transient film's kernels whose BinsView says "plane by emitter"; `planes` and
 * `stride` as planesLaunch takes them.  The table travels as the sensor's words, padded to whole floats with NONE. */
static wpt_status lightGroupsLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const uint8_t* groupOfMaterial,
        uint32_t materialCount, uint32_t groupCount, uint32_t envGroup, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size, float* frame, float* planes, size_t stride, hipStream_t stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame, stream };
    WPT_TRY(lightGroupsTable(groupOfMaterial, materialCount, groupCount, envGroup, rq.bins));
    if (!scene || !camera || !params || !planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (materialCount != uint32_t(scene->view.materialCount))
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the table has " + std::to_string(materialCount) + " materials, the scene "
                + std::to_string(uint32_t(scene->view.materialCount)));
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    rq.sensor = wptk::SENSOR_TRANSIENT;
    rq.bins.bins = planes;
    rq.bins.stride = stride;
    rq.bins.width = width;
    std::vector<float> words((size_t(materialCount) + 3) / 4 + 1);
    memset(words.data(), 0xff, words.size() * sizeof(float));
    memcpy(words.data(), groupOfMaterial, materialCount);
    return planesLaunch(rq, words.data(), words.size(), true, "light groups");
}

wpt_status wpt_render_light_groups_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count, uint32_t env_group, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* frame_device, float* planes_device, void* hip_stream)
{
    return lightGroupsLaunch(scene, camera, params, group_of_material, material_count, group_count, env_group, width, height, samples_sqrt,
            block_start, block_size, frame_device, planes_device, size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_light_groups_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count, uint32_t env_group, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb, float* block_planes)
{
    wptk::BinsView bv;
    WPT_TRY(lightGroupsTable(group_of_material, material_count, group_count, env_group, bv));
    if (!block_planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_planes is NULL");
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block, planes;
    if (block_rgb)
        HIP_TRY(block.allocatePixels(block_size));
    const hipError_t e = planes.allocatePixels(block_size, group_count);
    if (e != hipSuccess)
        return fail(WPT_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    return finishStaged(lightGroupsLaunch(scene, camera, params, group_of_material, material_count, group_count, env_group, width, height,
            samples_sqrt, block_start, block_size, block.biased(block_start), planes.biased(block_start), size_t(block_size) * 3, nullptr),
            scene, block, block_rgb, &planes, block_planes);
}

/* refuses a bad time-of-flight call before a device is needed */
static wpt_status tofCheck(const void* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor, const void* planes)
{
    if (!scene || !camera || !params || !sensor || !planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: NULL argument");
    if (sensor->phase_count == 0 || sensor->phase_count > WPT_TOF_MAX_PHASES)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: phase count must lie in 1 .. " + std::to_string(WPT_TOF_MAX_PHASES));
    bool finite = std::isfinite(sensor->pixel_area) && std::isfinite(sensor->exposure_time) && std::isfinite(sensor->contrast)
            && std::isfinite(sensor->frac_modfreq_c);
    for (uint32_t j = 0; j < sensor->phase_count; j++)
        finite = finite && std::isfinite(sensor->tau[j]);
    if (!finite)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: a sensor value is NaN or infinite");
    if (!(sensor->contrast >= 0.0f && sensor->contrast <= 1.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: contrast must lie in [0, 1]");
    if (params->min_dist_to_light != 0.0f || params->max_dist_to_light != FLT_MAX || params->min_path_len != 0.0f || params->max_path_len != FLT_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: it has no gates (the distance and path length gates must be the defaults)");
    return WPT_OK;
}

/* one time-of-flight launch.  One phase: the kernel keeps the taps in the pixel's accumulator and writes the plane as an RGB
 * launch writes its frame.  Several: the planes' block is zeroed, rendered into and scaled, all in stream order, as the
 * transient film's.  `planes` is plane 0's pixel 0 with `stride` floats between planes. */
static wpt_status tofLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* planes, size_t stride,
        hipStream_t stream)
{
    WPT_TRY(tofCheck(scene, camera, params, sensor, planes));
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    const uint32_t phases = sensor->phase_count;
    float consts[wpttof::C_TAU + WPT_TOF_MAX_PHASES] = {};
    consts[wpttof::C_PIXEL_AREA] = sensor->pixel_area;
    consts[wpttof::C_EXPOSURE_TIME] = sensor->exposure_time;
    consts[wpttof::C_CONTRAST] = sensor->contrast;
    consts[wpttof::C_FRAC_MODFREQ_C] = sensor->frac_modfreq_c;
    for (uint32_t j = 0; j < phases; j++)
        consts[wpttof::C_TAU + j] = sensor->tau[j];
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, phases == 1 ? planes : nullptr, stream };
    rq.sensor = wptk::SENSOR_TOF;
    rq.bins.bins = planes;
    rq.bins.stride = stride;
    rq.bins.binCount = phases;
    rq.bins.width = width;
    return planesLaunch(rq, consts, sizeof(consts) / sizeof(consts[0]), phases > 1, "time-of-flight sensor");
}

wpt_status wpt_render_tof_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* planes_device,
        void* hip_stream)
{
    return tofLaunch(scene, camera, params, sensor, width, height, samples_sqrt, block_start, block_size, planes_device,
            size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_tof_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_planes)
{
    WPT_TRY(tofCheck(scene, camera, params, sensor, block_planes));
    if (block_size == 0)
        return WPT_OK;
    StagedBlock planes;
    HIP_TRY(planes.allocatePixels(block_size, sensor->phase_count));
    return finishStaged(tofLaunch(scene, camera, params, sensor, width, height, samples_sqrt, block_start, block_size, planes.biased(block_start),
            size_t(block_size) * 3, nullptr), scene, planes, block_planes);
}

wpt_status wpt_tof_accumulate_host(const wpt_tof_sensor* sensor, uint32_t phase, float radiance_w, float opl_w, int is_tof_light, float acc[3])
{
    if (!sensor || !acc)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: NULL argument");
    if (sensor->phase_count == 0 || sensor->phase_count > WPT_TOF_MAX_PHASES || phase >= sensor->phase_count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: phase outside the sensor's phase count (1 .. " + std::to_string(WPT_TOF_MAX_PHASES) + ")");
    const float energy = wpttof::energy(sensor->pixel_area, sensor->exposure_time, radiance_w);
    const float t = is_tof_light ? wpttof::modulation(sensor->contrast, sensor->frac_modfreq_c, sensor->tau[phase], opl_w) : 0.0f;
    wpttof::add(energy, t, acc[0], acc[1], acc[2]);
    return WPT_OK;
}

/* what a batch of views is refused for before anything needs the scene or a device */
static wpt_status viewsCheck(const wpt_camera* cameras, uint32_t viewCount, const void* frames, uint32_t width, uint32_t height)
{
    if (viewCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: view_count is 0");
    if (!cameras)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: cameras are NULL");
    if (!frames)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: frames are NULL");
    for (uint32_t v = 0; v < viewCount; v++)
        if (cameras[v].animation < -1)
            return fail(WPT_ERR_INVALID_ARGUMENT, "views: camera " + std::to_string(v) + " refers to an animation outside the scene's array");
    /* the kernels index the batch's pixels, and hand them out from the pixel pool, in 32 bits */
    if (uint64_t(viewCount) * width * height > WPT_VIEWS_MAX_PIXELS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: view_count * width * height exceeds " + std::to_string(WPT_VIEWS_MAX_PIXELS) + " pixels");
    return WPT_OK;
}

/* what a batch of views is refused for: viewsCheck, and with the scene at hand what needs it */
static wpt_status viewsChecked(const wpt_scene* scene, const wpt_camera* cameras, uint32_t viewCount, const wpt_params* params, uint32_t width,
        uint32_t height, uint32_t samplesSqrt, const void* frames)
{
    WPT_TRY(viewsCheck(cameras, viewCount, frames, width, height));
    if (!scene || !params)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t v = 0; v < viewCount; v++)
        if (cameras[v].animation >= int32_t(scene->animationCount))
            return fail(WPT_ERR_INVALID_ARGUMENT, "views: camera " + std::to_string(v) + " refers to an animation outside the scene's array");
    return checkFrameBlock(width, height, &samplesSqrt, 0, 0);
}

/* the launch of a batch whose cameras and stream numbers (or NULL: all 0) are in device memory, written in stream order before
 * it; camerasHost: the same cameras, read for the launch's features */
static wpt_status viewsLaunch(wpt_scene* scene, const wpt_camera* camerasHost, const wpt_camera* camerasDevice, const uint32_t* streamsDevice,
        uint32_t viewCount, const wpt_params* params, uint32_t width, uint32_t height, uint32_t samplesSqrt, float* frames,
        wpt_counters* counters, void* hipStream)
{
    LaunchRequest rq = { scene, camerasHost, params, width, height, samplesSqrt, 0, viewCount * width * height, frames, hipStream };
    rq.counters = counters;
    rq.sensor = wptk::SENSOR_VIEWS;
    rq.views = { camerasDevice, width * height, viewCount, streamsDevice };
    return renderLaunch(rq);
}

wpt_status wpt_render_view_streams_device(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_device, wpt_counters* counters_device,
        void* hip_stream)
{
    WPT_TRY(viewsChecked(scene, cameras_host, view_count, params, width, height, samples_sqrt, frames_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* the cameras, and behind them the views' stream numbers, go to device memory once per batch, in stream order */
    const size_t camBytes = size_t(view_count) * sizeof(wpt_camera), streamBytes = streams_host ? size_t(view_count) * sizeof(uint32_t) : 0;
    static_assert(sizeof(wpt_camera) % alignof(uint32_t) == 0, "the stream numbers lie behind the cameras");
    StreamScratch scratch(stream);
    unsigned char* bytes = nullptr;
    WPT_TRY(hipStatus("views", scratch.get(camBytes + streamBytes, &bytes)));
    wpt_camera* dCams = reinterpret_cast<wpt_camera*>(bytes);
    uint32_t* dStreams = streams_host ? reinterpret_cast<uint32_t*>(dCams + view_count) : nullptr;
    hipError_t e = hipMemcpyAsync(dCams, cameras_host, camBytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && streams_host)
        e = hipMemcpyAsync(dStreams, streams_host, streamBytes, hipMemcpyHostToDevice, stream);
    WPT_TRY(hipStatus("views", e));
    return viewsLaunch(scene, cameras_host, dCams, dStreams, view_count, params, width, height, samples_sqrt, frames_device, counters_device,
            hip_stream);
}

wpt_status wpt_render_view_streams(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host)
{
    WPT_TRY(viewsCheck(cameras_host, view_count, frames_host, width, height));
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock frames;
    HIP_TRY(frames.allocatePixels(size_t(view_count) * width * height));
    return finishStaged(wpt_render_view_streams_device(scene, cameras_host, streams_host, view_count, params, width, height, samples_sqrt,
            frames.biased(0), nullptr, nullptr), scene, frames, frames_host);
}

wpt_status wpt_render_views_device(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_device, wpt_counters* counters_device, void* hip_stream)
{
    return wpt_render_view_streams_device(scene, cameras_host, nullptr, view_count, params, width, height, samples_sqrt, frames_device,
            counters_device, hip_stream);
}

wpt_status wpt_render_views(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host)
{
    return wpt_render_view_streams(scene, cameras_host, nullptr, view_count, params, width, height, samples_sqrt, frames_host);
}

/* what a split render is refused for before anything needs the scene or a device */
static wpt_status splitCheck(const wpt_camera* camera, uint32_t width, uint32_t height, uint32_t firstStream, uint32_t streamCount, const void* frame)
{
    if (streamCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: stream_count is 0");
    if (!camera)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: the camera is NULL");
    if (!frame)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: the frame is NULL");
    if (uint64_t(streamCount) * width * height > WPT_VIEWS_MAX_PIXELS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: stream_count * width * height exceeds " + std::to_string(WPT_VIEWS_MAX_PIXELS) + " pixels");
    if (uint64_t(firstStream) + streamCount > 0x100000000ull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: first_stream + stream_count exceeds 2^32");
    return WPT_OK;
}

wpt_status wpt_render_split_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_device, float* moments_device,
        wpt_counters* counters_device, void* hip_stream)
{
    WPT_TRY(splitCheck(camera, width, height, first_stream, stream_count, frame_device));
    /* the streams are a batch of views of one camera: view i is stream first_stream + i (the host's copies are read for the
     * launch's checks and features only, before this returns) */
    const std::vector<wpt_camera> cameras(stream_count, *camera);
    WPT_TRY(viewsChecked(scene, cameras.data(), stream_count, params, width, height, stream_samples_sqrt, frame_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* one allocation in stream order: the streams' frames, then their cameras and numbers, which a kernel writes (nothing
     * of the host's is read once the call has returned) */
    const size_t values = size_t(width) * height * 3, frameBytes = values * stream_count * sizeof(float);
    const size_t camBytes = size_t(stream_count) * sizeof(wpt_camera);
    static_assert(alignof(wpt_camera) <= alignof(float), "the cameras lie behind the streams' frames");
    static_assert(sizeof(wpt_camera) % sizeof(float) == 0, "the allocation is counted in floats");
    StreamScratch owner(stream);
    float* scratch = nullptr;
    WPT_TRY(hipStatus("split", owner.get((frameBytes + camBytes) / sizeof(float) + stream_count, &scratch)));
    wpt_camera* dCams = reinterpret_cast<wpt_camera*>(scratch + values * stream_count);
    uint32_t* dStreams = reinterpret_cast<uint32_t*>(dCams + stream_count);
    WPT_TRY(hipStatus("split", wptk::launchFillStreamViews(*camera, first_stream, stream_count, dCams, dStreams, stream)));
    WPT_TRY(viewsLaunch(scene, cameras.data(), dCams, dStreams, stream_count, params, width, height, stream_samples_sqrt, scratch, counters_device,
            hip_stream));
    return hipStatus("split", wptk::launchMeanPlanes(scratch, stream_count, values, values, frame_device, moments_device, stream));
}

wpt_status wpt_render_split(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_host, float* moments_host)
{
    WPT_TRY(splitCheck(camera, width, height, first_stream, stream_count, frame_host));
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock frame, moments;
    HIP_TRY(frame.allocatePixels(size_t(width) * height));
    if (moments_host)
        HIP_TRY(moments.allocatePixels(size_t(width) * height));
    return finishStaged(wpt_render_split_device(scene, camera, params, width, height, stream_samples_sqrt, first_stream, stream_count,
            frame.biased(0), moments.biased(0), nullptr, nullptr), scene, frame, frame_host, &moments, moments_host);
}

/* what an adaptive render is refused for before anything needs the scene or a device (every 16-bit count is valid) */
static wpt_status adaptiveCheck(uint32_t width, uint32_t height, const void* map, uint32_t blockStart, uint32_t blockSize, const void* frame)
{
    if (!map)
        return fail(WPT_ERR_INVALID_ARGUMENT, "adaptive: the sample-count map is NULL");
    if (!frame)
        return fail(WPT_ERR_INVALID_ARGUMENT, "adaptive: the frame is NULL");
    return checkFrameBlock(width, height, nullptr, blockStart, blockSize, 1, "adaptive: ");
}

wpt_status wpt_render_adaptive_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_device, uint32_t block_start, uint32_t block_size,
        float* frame_device, float* moments_device, void* hip_stream)
{
    WPT_TRY(adaptiveCheck(width, height, samples_sqrt_device, block_start, block_size, frame_device));
    /* (the launch's own samples_sqrt is unused by the adaptive kernels: 1 passes renderLaunch's checks) */
    LaunchRequest rq = { scene, camera, params, width, height, 1, block_start, block_size, frame_device, hip_stream };
    rq.sensor = wptk::SENSOR_ADAPTIVE;
    rq.adaptive = { samples_sqrt_device, moments_device };
    return renderLaunch(rq);
}

wpt_status wpt_render_adaptive_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_host, uint32_t block_start, uint32_t block_size,
        float* block_rgb, float* block_moments)
{
    WPT_TRY(adaptiveCheck(width, height, samples_sqrt_host, block_start, block_size, block_rgb));
    if (block_size == 0)
        return WPT_OK;
    /* device memory for the block only, behind pointers biased so that pixel `block_start` lands at offset 0; the caller's
     * values go there first, so that the pixels with n = 0 come back as they were */
    StagedBlock map, block, moments;
    hipError_t e = map.allocate(size_t(block_size) * sizeof(uint16_t));
    if (e == hipSuccess)
        e = block.allocatePixels(block_size);
    if (e == hipSuccess && block_moments)
        e = moments.allocatePixels(block_size);
    if (e == hipSuccess)
        e = map.upload(samples_sqrt_host + block_start);
    if (e == hipSuccess)
        e = block.upload(block_rgb);
    if (e == hipSuccess && block_moments)
        e = moments.upload(block_moments);
    WPT_TRY(hipStatus("adaptive", e, true));
    return finishStaged(wpt_render_adaptive_block_device(scene, camera, params, width, height, static_cast<uint16_t*>(map.device) - block_start,
            block_start, block_size, block.biased(block_start), moments.biased(block_start), nullptr), scene,
            block, block_rgb, &moments, block_moments);
}

} /* extern "C" */
