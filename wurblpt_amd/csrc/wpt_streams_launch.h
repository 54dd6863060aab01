/* wpt_streams_launch.h -- the launchers of wpt_k_streams.hip (wpt_postproc_mean_planes, _merge_means and wpt_render_split_device,
 * wpt_capi_sensors.hip, wpt_capi_postproc.hip) */
#ifndef WPT_STREAMS_LAUNCH_H
#define WPT_STREAMS_LAUNCH_H

#include <hip/hip_runtime.h>

#include "../../include/wurblpt_hip.h"
#include "wpt_streams.h"

namespace wptk {

/* lanes of a workgroup in the kernels of the unit: one value each */
constexpr uint32_t STREAMS_WG = 256;
/* values one launch takes: a grid of 2^31 - 1 workgroups */
constexpr uint64_t STREAMS_MAX_VALUES = 0x7fffffffull * STREAMS_WG;

/* Every pointer is device memory; one launch each, in stream order, no scratch.  values <= STREAMS_MAX_VALUES. */
hipError_t launchMeanPlanes(const float* planes, uint32_t planeCount, size_t stride, uint64_t values, float* mean, float* moment,
        hipStream_t stream);
/* cams[i] = camera and streams[i] = firstStream + i for i < count: the views of a split render (the camera travels as a kernel
 * argument, so nothing of the host's is read after the call) */
hipError_t launchFillStreamViews(const wpt_camera& camera, uint32_t firstStream, uint32_t count, wpt_camera* cams, uint32_t* streams,
        hipStream_t stream);
hipError_t launchMergeMeans(const float* a, uint32_t countA, const float* b, uint32_t countB, uint64_t values, float* out, hipStream_t stream);

}

#endif
