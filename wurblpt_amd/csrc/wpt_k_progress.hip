/* wpt_k_progress.hip -- the small kernels of a progressive session (wpt_capi.hip, wpt_progress_*): the preview of what the
 * pixels carry between stages, the frame's own order for a stage that resumes, and the finished frame kept in the carry.
 * One lane per pixel, no LDS; the path-tracing kernels are not touched by any of this. */
#include "wpt_progress.h"

namespace wptk {

namespace {

constexpr uint32_t PB = 256; /* threads per workgroup here */

inline dim3 gridFor(uint32_t blockSize)
{
    return dim3((uint32_t)(((uint64_t)blockSize + PB - 1) / PB));
}

/* lane -> pixel of the block; false behind its end (the index in 64 bits: a block may end at 2^32 - 1) */
__device__ inline bool blockPixel(uint32_t blockStart, uint32_t blockSize, size_t& p)
{
    const uint64_t gid = (uint64_t)blockIdx.x * PB + threadIdx.x;
    p = (size_t)blockStart + (size_t)gid;
    return gid < blockSize;
}

/* SensorRGB::finishPixel over the rows rendered so far: inv = 1.0f / (float)(rowsDone * samplesSqrt), divided on the host.
 * One 16-byte load of the pixel's SLOT_ACC quadword, three float stores that a wave lays side by side. */
__global__ __launch_bounds__(PB) void progress_resolve(const float4* __restrict__ carry, float* __restrict__ out, uint32_t blockStart,
        uint32_t blockSize, float inv)
{
    size_t p;
    if (!blockPixel(blockStart, blockSize, p))
        return;
    const float4 acc = carry[2 * p + 1];
    out[3 * p] = inv * acc.x;
    out[3 * p + 1] = inv * acc.y;
    out[3 * p + 2] = inv * acc.z;
}

__global__ __launch_bounds__(PB) void progress_frame_order(const KernelArgs args, uint32_t* __restrict__ order, uint32_t* __restrict__ count)
{
    const uint64_t gid = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (gid == 0)
        *count = args.blockSize;
    if (gid >= args.blockSize)
        return;
    uint32_t pixel;
    if (lanePixel(args, (uint32_t)gid, pixel))
        order[gid] = pixel;
}

__global__ __launch_bounds__(PB) void progress_capture(const float* __restrict__ frame, float4* __restrict__ carry, uint32_t blockStart,
        uint32_t blockSize, uint32_t stratum)
{
    size_t p;
    if (!blockPixel(blockStart, blockSize, p))
        return;
    carry[2 * p + 1] = make_float4(frame[3 * p], frame[3 * p + 1], frame[3 * p + 2], __uint_as_float(stratum));
}

}

void launchProgressResolve(const float4* carry, float* out, uint32_t blockStart, uint32_t blockSize, float inv, hipStream_t stream)
{
    hipLaunchKernelGGL(progress_resolve, gridFor(blockSize), dim3(PB), 0, stream, carry, out, blockStart, blockSize, inv);
}

void launchProgressFrameOrder(const KernelArgs& args, uint32_t* order, uint32_t* count, hipStream_t stream)
{
    hipLaunchKernelGGL(progress_frame_order, gridFor(args.blockSize), dim3(PB), 0, stream, args, order, count);
}

void launchProgressCapture(const float* frame, float4* carry, uint32_t blockStart, uint32_t blockSize, uint32_t stratum, hipStream_t stream)
{
    hipLaunchKernelGGL(progress_capture, gridFor(blockSize), dim3(PB), 0, stream, frame, carry, blockStart, blockSize, stratum);
}

}
