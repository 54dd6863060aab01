/* wpt_k_streams.hip -- the kernels of sample streams after the render (wpt_streams.h; wpt_postproc_mean_planes, _merge_means and
 * the reduce and the views of wpt_render_split_device in wpt_capi.hip).  One lane per float value: a wave reads 64 consecutive floats of a plane
 * (256 bytes, coalesced), the loop runs over the planes in order, and each lane runs the rule of wpt_streams.h that the host
 * loops run, so both write the same bits.  Nothing is reused, so the kernels are bound by the planes' bytes: K * values * 4 read,
 * values * 4 or 8 written.  No LDS, no scratch.  No path tracing in here; the path-tracing kernels are not touched by any of this. */
#include <hip/hip_runtime.h>

#include "wpt_streams_launch.h"

namespace wptk {

namespace {

__global__ __launch_bounds__(STREAMS_WG) void streams_mean_planes(const float* __restrict__ planes, uint32_t planeCount, size_t stride,
        uint64_t values, float* __restrict__ mean, float* __restrict__ moment)
{
    const uint64_t i = uint64_t(blockIdx.x) * STREAMS_WG + threadIdx.x;
    if (i >= values)
        return;
    /* (moment is the same in all lanes: the branch is uniform) */
    if (moment) {
        float m;
        mean[i] = wptstr::meanValue(planes, planeCount, stride, size_t(i), &m);
        moment[i] = m;
    } else {
        mean[i] = wptstr::meanValue(planes, planeCount, stride, size_t(i), nullptr);
    }
}

/* (out may be a or b: a lane reads and writes its own value only) */
__global__ __launch_bounds__(STREAMS_WG) void streams_merge_means(const float* a, uint32_t countA, const float* b, uint32_t countB,
        uint64_t values, float* out)
{
    const uint64_t i = uint64_t(blockIdx.x) * STREAMS_WG + threadIdx.x;
    if (i < values)
        out[i] = wptstr::mergeValue(a[i], countA, b[i], countB);
}

/* the views of a split render: one lane per view */
__global__ __launch_bounds__(STREAMS_WG) void streams_fill_views(const wpt_camera camera, uint32_t firstStream, uint32_t count,
        wpt_camera* __restrict__ cams, uint32_t* __restrict__ streams)
{
    const uint32_t i = blockIdx.x * STREAMS_WG + threadIdx.x;
    if (i < count) {
        cams[i] = camera;
        streams[i] = firstStream + i;
    }
}

uint32_t workgroups(uint64_t values)
{
    return uint32_t((values + STREAMS_WG - 1) / STREAMS_WG);
}

} /* namespace */

hipError_t launchMeanPlanes(const float* planes, uint32_t planeCount, size_t stride, uint64_t values, float* mean, float* moment,
        hipStream_t stream)
{
    if (values == 0 || values > STREAMS_MAX_VALUES || planeCount == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(streams_mean_planes, dim3(workgroups(values)), dim3(STREAMS_WG), 0, stream, planes, planeCount, stride, values, mean,
            moment);
    return hipGetLastError();
}

hipError_t launchFillStreamViews(const wpt_camera& camera, uint32_t firstStream, uint32_t count, wpt_camera* cams, uint32_t* streams,
        hipStream_t stream)
{
    if (count == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(streams_fill_views, dim3(workgroups(count)), dim3(STREAMS_WG), 0, stream, camera, firstStream, count, cams, streams);
    return hipGetLastError();
}

hipError_t launchMergeMeans(const float* a, uint32_t countA, const float* b, uint32_t countB, uint64_t values, float* out, hipStream_t stream)
{
    if (values == 0 || values > STREAMS_MAX_VALUES || uint64_t(countA) + countB == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(streams_merge_means, dim3(workgroups(values)), dim3(STREAMS_WG), 0, stream, a, countA, b, countB, values, out);
    return hipGetLastError();
}

}
