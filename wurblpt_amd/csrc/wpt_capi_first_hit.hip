/*
 * wpt_capi_first_hit.hip -- of include/wurblpt_hip.h: the two passes that walk one ray per pixel to its first hit,
 * wpt_ground_truth(_device) (kernels: wpt_k_groundtruth.hip) and wpt_first_hit_colours(_device) (wpt_k_firsthit.hip).
 */
#include "wpt_capi_common.h"
#include "wpt_firsthit_launch.h"
#include "wpt_denoise.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

extern "C" {

wpt_status wpt_ground_truth_device(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_device[WPT_GT_ARRAY_COUNT], void* hip_stream)
{
    if (!scene || !camera || !params || !arrays_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width == 0 || height == 0 || uint64_t(width) * height > 0xffffffffull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (camera->surround_mode > WPT_SURROUND_360)
        return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
    if ((arrays_device[WPT_GT_PIXEL_SPACE_OFFSET_TO_PREV] || arrays_device[WPT_GT_PIXEL_SPACE_OFFSET_TO_NEXT])
            && (camera->surround_mode != WPT_SURROUND_OFF || camera->stereoscopic_distance > 0.0f))
        return fail(WPT_ERR_UNSUPPORTED, "pixel space offsets exist for Surround_Off, non-stereoscopic cameras only (camera.hpp:207-208)");
    GroundTruthArgs args;
    args.scene = scene->view;
    args.cam = *camera;
    args.camPrev = camera_prev ? *camera_prev : *camera;
    args.camNext = camera_next ? *camera_next : *camera;
    args.par = *params;
    args.t0 = times ? times[0] : 0.0f;
    args.tPrev = times ? times[1] : 0.0f;
    args.tNext = times ? times[2] : 0.0f;
    args.par.t0 = args.par.t1 = args.t0; /* one moment, no exposure interval */
    args.width = width;
    args.height = height;
    bool any = false;
    for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++) {
        args.array[k] = arrays_device[k];
        any = any || arrays_device[k];
    }
    if (!any)
        return WPT_OK;
    launchGroundTruth(args, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_ground_truth(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_host[WPT_GT_ARRAY_COUNT])
{
    if (!arrays_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const size_t pixels = size_t(width) * height;
    StagedBlock staged[WPT_GT_ARRAY_COUNT];
    void* dev[WPT_GT_ARRAY_COUNT];
    for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++) {
        if (arrays_host[k] && pixels > 0)
            WPT_TRY(hipStatus("hipMalloc", staged[k].allocate(pixels * wpt_gt_components[k] * 4), true));
        dev[k] = staged[k].device;
    }
    WPT_TRY(wpt_ground_truth_device(scene, camera, camera_prev, camera_next, times, params, width, height, dev, nullptr));
    hipError_t e = hipDeviceSynchronize();
    for (int k = 0; k < WPT_GT_ARRAY_COUNT && e == hipSuccess; k++)
        e = staged[k].download(arrays_host[k]);
    return hipStatus("ground truth", e);
}

/* what a first-hit colour pass is refused for, before a device is needed; `out`: albedo, emission and the three guide arrays */
static wpt_status firstHitCheck(const wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        void* const out[5])
{
    if (!scene || !camera || !params)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: NULL argument");
    if (width == 0 || height == 0 || width > wptdn::SIDE_MAX || height > wptdn::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: width and height must lie in 1 .. " + std::to_string(uint32_t(wptdn::SIDE_MAX)));
    const size_t pixels = size_t(width) * height;
    const size_t bytes[5] = { pixels * 12, pixels * 12, pixels * 12, pixels * 12, pixels * 4 };
    bool any = false;
    for (int k = 0; k < 5; k++) {
        any = any || out[k];
        for (int j = 0; j < k; j++) {
            if (out[k] && out[j] && overlaps(out[k], bytes[k], out[j], bytes[j]))
                return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: two outputs overlap");
        }
    }
    if (!any)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: no output is wanted (all five arrays are NULL)");
    if (camera->surround_mode > WPT_SURROUND_360)
        return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
    return WPT_OK;
}

wpt_status wpt_first_hit_colours_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width,
        uint32_t height, float* albedo_device, float* emission_device, void* const guide_device[3], void* hip_stream)
{
    void* const out[5] = { albedo_device, emission_device, guide_device ? guide_device[0] : nullptr, guide_device ? guide_device[1] : nullptr,
        guide_device ? guide_device[2] : nullptr };
    WPT_TRY(firstHitCheck(scene, camera, params, width, height, out));
    wptk::FirstHitArgs args;
    args.scene = scene->view;
    args.cam = *camera;
    args.par = *params;
    args.par.t1 = args.par.t0; /* one moment, no exposure interval */
    args.width = width;
    args.height = height;
    args.albedo = albedo_device;
    args.emission = emission_device;
    args.positions = static_cast<float*>(out[2]);
    args.normals = static_cast<float*>(out[3]);
    args.materials = static_cast<int32_t*>(out[4]);
    wptk::launchFirstHitColours(args, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_first_hit_colours(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        float* albedo_host, float* emission_host, void* const guide_host[3])
{
    void* const host[5] = { albedo_host, emission_host, guide_host ? guide_host[0] : nullptr, guide_host ? guide_host[1] : nullptr,
        guide_host ? guide_host[2] : nullptr };
    WPT_TRY(firstHitCheck(scene, camera, params, width, height, host));
    const size_t pixels = size_t(width) * height;
    const size_t bytes[5] = { pixels * 12, pixels * 12, pixels * 12, pixels * 12, pixels * 4 };
    StagedBlock staged[5];
    void* dev[5];
    for (int k = 0; k < 5; k++) {
        if (host[k])
            WPT_TRY(hipStatus("hipMalloc", staged[k].allocate(bytes[k]), true));
        dev[k] = staged[k].device;
    }
    WPT_TRY(wpt_first_hit_colours_device(scene, camera, params, width, height, static_cast<float*>(dev[0]), static_cast<float*>(dev[1]), dev + 2,
            nullptr));
    hipError_t e = hipDeviceSynchronize();
    for (int k = 0; k < 5 && e == hipSuccess; k++)
        e = staged[k].download(host[k]);
    return hipStatus("first-hit colours", e);
}

} /* extern "C" */
