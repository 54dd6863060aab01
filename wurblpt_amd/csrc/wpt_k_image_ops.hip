/* wpt_k_image_ops.hip -- the kernels of the output side's image operations (wpt_image_ops.h; wpt_postproc_resample, _lens_warp,
 * _despeckle and _distance_to_coords in wpt_capi.hip).  One lane per output pixel, a workgroup is 32 x 8 of them; each lane runs
 * the rule of wpt_image_ops.h that the host loops run, so both write the same bits.  The four taps of a bilinear look-up are
 * plain loads (the L2 serves the reuse between neighbours); the iterative inverse of the OpenCV lens model is the out-of-line
 * wptlens::undistortCall, so a wave whose lanes need different iteration counts runs as long as its slowest lane.
 * Despeckle has two forms that run the same wptio::despecklePixel:
 *   gather  every lane loads its nine pixels from device memory
 *   tile    a workgroup first copies its 32 x 8 pixels and the ring around them into LDS (4 KB) and reads the nine there
 * Which one a call takes is WPT_DESPECKLE_TILE.  Measured (profiles/image_ops_rate.txt, three alternating repeats): both take 11.4 us
 * at 1024 x 1024; at 3840 x 2160 the tile form takes 66.7 us against 69.2 us (spreads 0.3 and 0.5 %), so the tile form it is.
 * No path tracing in here; the path-tracing kernels are not touched by any of this. */
#include <hip/hip_runtime.h>

#include "wpt_image_ops_launch.h"

/* 1: despeckle takes the tile form, 0: the gather form */
#ifndef WPT_DESPECKLE_TILE
#define WPT_DESPECKLE_TILE 1
#endif

namespace wptk {

namespace {

using wptio::Image;
using wptlens::Coeffs;

constexpr int TW = int(IMAGE_OPS_TILE_W), TH = int(IMAGE_OPS_TILE_H);
constexpr int RING_W = TW + 2, RING_H = TH + 2; /* the tile and the ring of neighbours around it */

__global__ __launch_bounds__(TW * TH) void image_resample(const Image img, uint32_t newWidth, uint32_t newHeight, float* __restrict__ out)
{
    const uint32_t x = blockIdx.x * TW + threadIdx.x;
    const uint32_t y = blockIdx.y * TH + threadIdx.y;
    if (x >= newWidth || y >= newHeight)
        return;
    wptio::resamplePixel(img, x, y, newWidth, newHeight, out + (size_t(y) * newWidth + x) * img.comps);
}

__global__ __launch_bounds__(TW * TH) void image_lens_warp(const Image img, const Coeffs lens, bool forward, float* __restrict__ out)
{
    const uint32_t x = blockIdx.x * TW + threadIdx.x;
    const uint32_t y = blockIdx.y * TH + threadIdx.y;
    if (x >= img.width || y >= img.height)
        return;
    wptio::warpPixel(img, lens, forward, x, y, out + (size_t(y) * img.width + x) * img.comps);
}

__global__ __launch_bounds__(TW * TH) void image_distance_to_coords(const Image img, const Coeffs lens, bool pmdSpace, float* __restrict__ out)
{
    const uint32_t x = blockIdx.x * TW + threadIdx.x;
    const uint32_t y = blockIdx.y * TH + threadIdx.y;
    if (x >= img.width || y >= img.height)
        return;
    wptio::coordsPixel(img, lens, pmdSpace, x, y, out + (size_t(y) * img.width + x) * 3);
}

__global__ __launch_bounds__(TW * TH) void image_despeckle_gather(const float* __restrict__ rgb, int width, int height, float minFactor,
        float* __restrict__ out)
{
    const int x = (int)blockIdx.x * TW + (int)threadIdx.x;
    const int y = (int)blockIdx.y * TH + (int)threadIdx.y;
    if (x >= width || y >= height)
        return;
    const wptio::ClampFetch fetch = { rgb, width, height };
    wptio::despecklePixel(fetch, x, y, minFactor, out + (size_t(y) * size_t(width) + size_t(x)) * 3);
}

/* a workgroup's tile and ring in LDS: pixel (xx, yy), before clamping, lies at (xx - x0, yy - y0); the copy clamped already */
struct RingFetch {
    const float* ring;
    int x0, y0;
    __device__ void rgb(int xx, int yy, float* v) const
    {
        const float* p = ring + ((yy - y0) * RING_W + (xx - x0)) * 3;
        v[0] = p[0];
        v[1] = p[1];
        v[2] = p[2];
    }
};

__global__ __launch_bounds__(TW * TH) void image_despeckle_tile(const float* __restrict__ rgb, int width, int height, float minFactor,
        float* __restrict__ out)
{
    __shared__ float ring[RING_W * RING_H * 3];
    const int x0 = (int)blockIdx.x * TW - 1;
    const int y0 = (int)blockIdx.y * TH - 1;
    const int lane = (int)threadIdx.y * TW + (int)threadIdx.x;
    const wptio::ClampFetch global = { rgb, width, height };
    for (int i = lane; i < RING_W * RING_H; i += TW * TH)
        global.rgb(x0 + i % RING_W, y0 + i / RING_W, ring + i * 3);
    __syncthreads();
    const int x = (int)blockIdx.x * TW + (int)threadIdx.x;
    const int y = (int)blockIdx.y * TH + (int)threadIdx.y;
    if (x >= width || y >= height)
        return;
    const RingFetch fetch = { ring, x0, y0 };
    wptio::despecklePixel(fetch, x, y, minFactor, out + (size_t(y) * size_t(width) + size_t(x)) * 3);
}

dim3 tilesOf(uint32_t width, uint32_t height)
{
    return dim3((width + IMAGE_OPS_TILE_W - 1) / IMAGE_OPS_TILE_W, (height + IMAGE_OPS_TILE_H - 1) / IMAGE_OPS_TILE_H);
}

}

bool despeckleTileByDefault()
{
    return WPT_DESPECKLE_TILE != 0;
}

hipError_t launchResample(const Image& img, uint32_t newWidth, uint32_t newHeight, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(image_resample, tilesOf(newWidth, newHeight), dim3(TW, TH), 0, stream, img, newWidth, newHeight, out);
    return hipGetLastError();
}

hipError_t launchLensWarp(const Image& img, const Coeffs& lens, bool forward, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(image_lens_warp, tilesOf(img.width, img.height), dim3(TW, TH), 0, stream, img, lens, forward, out);
    return hipGetLastError();
}

hipError_t launchDistanceToCoords(const Image& img, const Coeffs& lens, bool pmdSpace, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(image_distance_to_coords, tilesOf(img.width, img.height), dim3(TW, TH), 0, stream, img, lens, pmdSpace, out);
    return hipGetLastError();
}

hipError_t launchDespeckle(const float* rgb, uint32_t width, uint32_t height, float minFactor, bool tile, float* out, hipStream_t stream)
{
    if (tile)
        hipLaunchKernelGGL(image_despeckle_tile, tilesOf(width, height), dim3(TW, TH), 0, stream, rgb, int(width), int(height), minFactor, out);
    else
        hipLaunchKernelGGL(image_despeckle_gather, tilesOf(width, height), dim3(TW, TH), 0, stream, rgb, int(width), int(height), minFactor, out);
    return hipGetLastError();
}

}
