/* wpt_k_temporal.hip -- the kernel of temporal accumulation (wpt_temporal.h; wpt_postproc_temporal_accumulate in
 * wpt_capi_postproc.hip): one lane per pixel makes the pixel's records from the render's outputs (wptdn::prepare, which takes the
 * place of denoise_pack), gathers up to four taps of the previous history and writes the three records of the new one.  Every
 * record access is one 16-byte access per lane; the planes make a wave's own-pixel reads and writes 1 KiB contiguous per
 * instruction.  The taps are a gather that the L2 serves: the offsets differ per pixel.  No path tracing in here. */
#include <hip/hip_runtime.h>

#include "wpt_temporal_launch.h"

namespace wptk {

namespace {

using wptdn::Rec;

constexpr uint32_t TB = 256; /* threads per workgroup: one lane per pixel, in the order of the arrays */

__global__ __launch_bounds__(TB) void temporal_accumulate(const float* __restrict__ frame, const float* __restrict__ moments,
        const uint16_t* __restrict__ samplesSqrt, const float* __restrict__ positions, const float* __restrict__ normals,
        const int32_t* __restrict__ materials, const float* __restrict__ pixelOffsets, const float* __restrict__ cameraOffsets,
        const Rec* __restrict__ prev, uint32_t width, uint32_t height, const wpttm::Params params, Rec* __restrict__ out,
        float* __restrict__ lengthOut)
{
    const size_t pixels = size_t(width) * height;
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p >= pixels)
        return;
    const uint32_t y = uint32_t(p / width);
    const uint32_t x = uint32_t(p - size_t(y) * width);
    const uint32_t n = samplesSqrt[p];
    Rec A, B, C, newB, newC;
    wptdn::prepare(frame + 3 * p, moments + 3 * p, n, positions + 3 * p, normals + 3 * p, materials[p], A, B, C);
    const wpttm::History history(prev ? prev : out, width, pixels); /* never read without `prev` */
    wpttm::accumulatePixel(A, B, C, n, prev ? &history : nullptr, pixelOffsets ? pixelOffsets + 2 * p : nullptr,
            cameraOffsets ? cameraOffsets + 3 * p : nullptr, int(x), int(y), int(width), int(height), params, newB, newC);
    out[p] = A;
    out[pixels + p] = newB;
    out[2 * pixels + p] = newC;
    if (lengthOut)
        lengthOut[p] = newB.w;
}

}

hipError_t launchTemporalAccumulate(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions,
        const float* normals, const int32_t* materials, const float* pixelOffsets, const float* cameraOffsets, const wptdn::Rec* prev,
        uint32_t width, uint32_t height, const wpttm::Params& params, wptdn::Rec* out, float* lengthOut, hipStream_t stream)
{
    const size_t pixels = size_t(width) * height;
    hipLaunchKernelGGL(temporal_accumulate, dim3((uint32_t)((pixels + TB - 1) / TB)), dim3(TB), 0, stream, frame, moments, samplesSqrt, positions,
            normals, materials, pixelOffsets, cameraOffsets, prev, width, height, params, out, lengthOut);
    return hipGetLastError();
}

}
