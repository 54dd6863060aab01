/* wpt_k_denoise.hip -- the kernels of the spatial denoiser (wpt_denoise.h; wpt_postproc_denoise in wpt_capi.hip): pack the
 * render's outputs into 16-byte records (plain, or demodulated by the first-hit colours), one launch per iteration over two colour buffers, unpack the result.  A tap is three
 * 16-byte loads.  An iteration has two forms that run the same wptdn::filterPixel and so write the same bits:
 *   gather  every lane reads its 25 taps from device memory (the L2 serves the reuse between neighbours)
 *   tile    a workgroup first copies its 32 x 16 pixels and their halo of 2 * step records into LDS and reads the taps there
 * Which form a step takes is ldsFormForStep(): decided from the step alone (profiles/denoise_rate.txt has the measurement).
 * No path tracing in here; the path-tracing kernels are not touched by any of this. */
#include <hip/hip_runtime.h>

#include "wpt_denoise_launch.h"
#include "wpt_temporal_launch.h"

/* the largest step that takes the tile form; 0: none.  At most 2: the tile of step 4 would need 72 KB.  (A second build with
 * EXTRA=-DWPT_DENOISE_LDS_MAX_STEP=... is how tools/denoise_rate.py measures one form against the other.) */
#ifndef WPT_DENOISE_LDS_MAX_STEP
#define WPT_DENOISE_LDS_MAX_STEP 2
#endif

namespace wptk {

namespace {

using wptdn::Params;
using wptdn::Rec;

constexpr uint32_t PB = 256;                    /* threads per workgroup of pack and unpack: one lane per pixel */
constexpr int TILE_W = 32, TILE_H = 16;         /* a workgroup's pixels in an iteration: one lane each */
constexpr int LDS_MAX_STEP = WPT_DENOISE_LDS_MAX_STEP;
constexpr int LDS_HALO = 2 * (LDS_MAX_STEP > 0 ? LDS_MAX_STEP : 1);
constexpr int LDS_RECORDS = (TILE_W + 2 * LDS_HALO) * (TILE_H + 2 * LDS_HALO); /* per array, at the largest step in LDS */
static_assert(LDS_MAX_STEP >= 0 && LDS_MAX_STEP <= 2, "the tile and its halo must fit 64 KB of LDS");
static_assert(size_t(LDS_RECORDS) * 3 * sizeof(Rec) <= 65536, "the tile and its halo must fit 64 KB of LDS");

inline bool ldsFormForStep(int step)
{
    return step <= LDS_MAX_STEP;
}

__global__ __launch_bounds__(PB) void denoise_pack(const float* __restrict__ frame, const float* __restrict__ moments,
        const uint16_t* __restrict__ samplesSqrt, const float* __restrict__ positions, const float* __restrict__ normals,
        const int32_t* __restrict__ materials, size_t pixels, Rec* __restrict__ guideA, Rec* __restrict__ guideB, Rec* __restrict__ colour)
{
    const size_t p = (size_t)blockIdx.x * PB + threadIdx.x;
    if (p >= pixels)
        return;
    Rec a, b, c;
    wptdn::prepare(frame + 3 * p, moments + 3 * p, samplesSqrt[p], positions + 3 * p, normals + 3 * p, materials[p], a, b, c);
    guideA[p] = a;
    guideB[p] = b;
    colour[p] = c;
}

__global__ __launch_bounds__(PB) void denoise_unpack(const Rec* __restrict__ colour, size_t pixels, float* __restrict__ out,
        float* __restrict__ variance)
{
    const size_t p = (size_t)blockIdx.x * PB + threadIdx.x;
    if (p >= pixels)
        return;
    const Rec c = colour[p];
    out[3 * p] = c.x;
    out[3 * p + 1] = c.y;
    out[3 * p + 2] = c.z;
    if (variance)
        variance[p] = c.w;
}

/* pack and unpack of the demodulated form (wpt_denoise.h, prepareDemodulated / finishDemodulated); the iterations between them
 * are the kernels below, unchanged */
__global__ __launch_bounds__(PB) void denoise_pack_demodulated(const float* __restrict__ frame, const float* __restrict__ moments,
        const uint16_t* __restrict__ samplesSqrt, const float* __restrict__ positions, const float* __restrict__ normals,
        const int32_t* __restrict__ materials, const float* __restrict__ albedo, const float* __restrict__ emission, float albedoFloor,
        size_t pixels, Rec* __restrict__ guideA, Rec* __restrict__ guideB, Rec* __restrict__ colour)
{
    const size_t p = (size_t)blockIdx.x * PB + threadIdx.x;
    if (p >= pixels)
        return;
    Rec a, b, c;
    wptdn::prepareDemodulated(frame + 3 * p, moments + 3 * p, samplesSqrt[p], positions + 3 * p, normals + 3 * p, materials[p], albedo + 3 * p,
            emission + 3 * p, albedoFloor, a, b, c);
    guideA[p] = a;
    guideB[p] = b;
    colour[p] = c;
}

__global__ __launch_bounds__(PB) void denoise_unpack_demodulated(const Rec* __restrict__ colour, const float* __restrict__ albedo,
        const float* __restrict__ emission, float albedoFloor, size_t pixels, float* __restrict__ out, float* __restrict__ variance)
{
    const size_t p = (size_t)blockIdx.x * PB + threadIdx.x;
    if (p >= pixels)
        return;
    const Rec c = colour[p];
    float rgb[3];
    wptdn::finishDemodulated(c, albedo + 3 * p, emission + 3 * p, albedoFloor, rgb);
    out[3 * p] = rgb[0];
    out[3 * p + 1] = rgb[1];
    out[3 * p + 2] = rgb[2];
    if (variance)
        variance[p] = c.w;
}

/* a frame's records in device memory */
struct GlobalFetch {
    const Rec* a;
    const Rec* b;
    const Rec* c;
    size_t width;
    __device__ Rec guideA(int x, int y) const { return a[size_t(y) * width + size_t(x)]; }
    __device__ Rec guideB(int x, int y) const { return b[size_t(y) * width + size_t(x)]; }
    __device__ Rec colour(int x, int y) const { return c[size_t(y) * width + size_t(x)]; }
};

/* a workgroup's tile and halo in LDS: record (x, y) of the frame lies at (x - x0, y - y0) of rows of `pitch` records */
struct TileFetch {
    const Rec* a;
    const Rec* b;
    const Rec* c;
    int x0, y0, pitch;
    __device__ int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
    __device__ Rec guideA(int x, int y) const { return a[at(x, y)]; }
    __device__ Rec guideB(int x, int y) const { return b[at(x, y)]; }
    __device__ Rec colour(int x, int y) const { return c[at(x, y)]; }
};

__global__ __launch_bounds__(TILE_W * TILE_H) void denoise_iterate_gather(const Rec* __restrict__ guideA, const Rec* __restrict__ guideB,
        const Rec* __restrict__ from, Rec* __restrict__ to, int width, int height, int step, const Params params)
{
    const int x = (int)blockIdx.x * TILE_W + (int)threadIdx.x;
    const int y = (int)blockIdx.y * TILE_H + (int)threadIdx.y;
    if (x >= width || y >= height)
        return;
    const GlobalFetch fetch = { guideA, guideB, from, size_t(width) };
    to[size_t(y) * size_t(width) + size_t(x)] = wptdn::filterPixel(fetch, x, y, width, height, step, params);
}

/* step <= LDS_MAX_STEP only (the launcher sees to it): the tile's rows are TILE_W + 4 * step records, TILE_H + 4 * step of them.
 * Records outside the frame are not copied and never read: filterPixel skips a tap by its coordinates. */
__global__ __launch_bounds__(TILE_W * TILE_H) void denoise_iterate_tile(const Rec* __restrict__ guideA, const Rec* __restrict__ guideB,
        const Rec* __restrict__ from, Rec* __restrict__ to, int width, int height, int step, const Params params)
{
    __shared__ Rec tile[3][LDS_RECORDS];
    const int halo = 2 * step;
    const int pitch = TILE_W + 2 * halo;
    const int rows = TILE_H + 2 * halo;
    const int x0 = (int)blockIdx.x * TILE_W - halo;
    const int y0 = (int)blockIdx.y * TILE_H - halo;
    const int lane = (int)threadIdx.y * TILE_W + (int)threadIdx.x;
    const int records = pitch * rows < LDS_RECORDS ? pitch * rows : LDS_RECORDS;
    for (int i = lane; i < records; i += TILE_W * TILE_H) {
        const int gx = x0 + i % pitch;
        const int gy = y0 + i / pitch;
        if (gx < 0 || gy < 0 || gx >= width || gy >= height)
            continue;
        const size_t p = size_t(gy) * size_t(width) + size_t(gx);
        tile[0][i] = guideA[p];
        tile[1][i] = guideB[p];
        tile[2][i] = from[p];
    }
    __syncthreads();
    const int x = (int)blockIdx.x * TILE_W + (int)threadIdx.x;
    const int y = (int)blockIdx.y * TILE_H + (int)threadIdx.y;
    if (x >= width || y >= height)
        return;
    const TileFetch fetch = { tile[0], tile[1], tile[2], x0, y0, pitch };
    to[size_t(y) * size_t(width) + size_t(x)] = wptdn::filterPixel(fetch, x, y, width, height, step, params);
}

}

const char* denoiseFormOfStep(uint32_t step)
{
    return ldsFormForStep(int(step)) ? "tile" : "gather";
}

namespace {

/* the iterations in stream order; returns the buffer that holds the result */
Rec* launchIterations(const Rec* a, const Rec* b, Rec* from, Rec* to, uint32_t width, uint32_t height, const Params& params, uint32_t iterations,
        hipStream_t stream)
{
    const dim3 tiles((width + TILE_W - 1) / TILE_W, (height + TILE_H - 1) / TILE_H);
    for (uint32_t i = 0; i < iterations; i++) {
        const int step = 1 << i;
        if (ldsFormForStep(step))
            hipLaunchKernelGGL(denoise_iterate_tile, tiles, dim3(TILE_W, TILE_H), 0, stream, a, b, from, to, int(width), int(height), step, params);
        else
            hipLaunchKernelGGL(denoise_iterate_gather, tiles, dim3(TILE_W, TILE_H), 0, stream, a, b, from, to, int(width), int(height), step, params);
        Rec* t = from;
        from = to;
        to = t;
    }
    return from;
}

}

hipError_t launchDenoise(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions, const float* normals,
        const int32_t* materials, uint32_t width, uint32_t height, const wptdn::Params& params, uint32_t iterations, wptdn::Rec* scratch,
        float* out, float* variance, hipStream_t stream)
{
    const size_t pixels = size_t(width) * height;
    Rec* a = scratch;
    Rec* b = scratch + pixels;
    Rec* from = scratch + 2 * pixels;
    const dim3 perPixel((uint32_t)((pixels + PB - 1) / PB));
    hipLaunchKernelGGL(denoise_pack, perPixel, dim3(PB), 0, stream, frame, moments, samplesSqrt, positions, normals, materials, pixels, a, b, from);
    from = launchIterations(a, b, from, scratch + 3 * pixels, width, height, params, iterations, stream);
    hipLaunchKernelGGL(denoise_unpack, perPixel, dim3(PB), 0, stream, from, pixels, out, variance);
    return hipGetLastError();
}

hipError_t launchDenoiseDemodulated(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions,
        const float* normals, const int32_t* materials, const float* albedo, const float* emission, uint32_t width, uint32_t height,
        const wptdn::Params& params, uint32_t iterations, float albedoFloor, wptdn::Rec* scratch, float* out, float* variance, hipStream_t stream)
{
    const size_t pixels = size_t(width) * height;
    Rec* a = scratch;
    Rec* b = scratch + pixels;
    Rec* from = scratch + 2 * pixels;
    const dim3 perPixel((uint32_t)((pixels + PB - 1) / PB));
    hipLaunchKernelGGL(denoise_pack_demodulated, perPixel, dim3(PB), 0, stream, frame, moments, samplesSqrt, positions, normals, materials, albedo,
            emission, albedoFloor, pixels, a, b, from);
    from = launchIterations(a, b, from, scratch + 3 * pixels, width, height, params, iterations, stream);
    hipLaunchKernelGGL(denoise_unpack_demodulated, perPixel, dim3(PB), 0, stream, from, albedo, emission, albedoFloor, pixels, out, variance);
    return hipGetLastError();
}

/* the filter on a history (wpt_temporal.h): the guides and the first iteration's colours are the history's planes, which no
 * iteration writes; no pack */
hipError_t launchDenoiseHistory(const wptdn::Rec* history, uint32_t width, uint32_t height, const wptdn::Params& params, uint32_t iterations,
        wptdn::Rec* scratch, float* out, float* variance, hipStream_t stream)
{
    const size_t pixels = size_t(width) * height;
    const Rec* a = history;
    const Rec* b = history + pixels;
    const Rec* from = history + 2 * pixels;
    const dim3 tiles((width + TILE_W - 1) / TILE_W, (height + TILE_H - 1) / TILE_H);
    for (uint32_t i = 0; i < iterations; i++) {
        const int step = 1 << i;
        Rec* to = scratch + (i & 1u) * pixels;
        if (ldsFormForStep(step))
            hipLaunchKernelGGL(denoise_iterate_tile, tiles, dim3(TILE_W, TILE_H), 0, stream, a, b, from, to, int(width), int(height), step, params);
        else
            hipLaunchKernelGGL(denoise_iterate_gather, tiles, dim3(TILE_W, TILE_H), 0, stream, a, b, from, to, int(width), int(height), step, params);
        from = to;
    }
    const dim3 perPixel((uint32_t)((pixels + PB - 1) / PB));
    hipLaunchKernelGGL(denoise_unpack, perPixel, dim3(PB), 0, stream, from, pixels, out, variance);
    return hipGetLastError();
}

}
