/*
 * wpt_temporal.h -- temporal accumulation in front of the spatial denoiser (wpt_denoise.h): a pixel's estimate is carried from
 * frame to frame along the motion the ground truth pass writes, so that F frames of n samples count as F * n samples where a
 * surface stays visible.  Restated in float, operation for operation, every product and sum rounded on its own
 * (-ffp-contract=off), so that the device and the host give the same bits.  include/wurblpt_hip.h holds the rule.
 *
 * A history is the filter's own three 16-byte records per pixel, kept: planes [3][height][width] of wptdn::Rec,
 *   plane 0  guide A = P.xyz and the bits of m            (what validates a reprojection)
 *   plane 1  guide B = n.xyz, and in w the history length N as a float (filterPixel reads B only through dot3: w is free)
 *   plane 2  colour  = the accumulated rgb, and in w the variance of its luminance
 * accumulatePixel() makes a pixel's new records from prepare()'s records of the current frame and up to four taps of the
 * previous history; `History` says where a history's records lie.  The filter's iterations then run on a history as it is.
 * The normals compared are camera-space normals of two different frames: a camera that turns between frames turns a static
 * surface's normal with it, so normalCosMin has to cover that turn.
 * Written once; compiled for the device (wpt_k_temporal.hip), for the host (wpt_postproc_temporal_accumulate_host) and, outside
 * the library and without a header of HIP, by tests/temporal_check.cpp.
 */
#ifndef WPT_TEMPORAL_H
#define WPT_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#include "wpt_denoise.h"

namespace wpttm {

using wptdn::Rec;

enum : uint32_t {
    HISTORY_PLANES = 3u,                       /* guide A, guide B (w = N), colour (w = V) */
    HISTORY_BYTES_PER_PIXEL = 3u * sizeof(Rec) /* 48 */
};

/* wpt_temporal_params with the tolerance's square taken once */
struct Params {
    float maxHistory;
    float normalCosMin;
    float tolerance2; /* position_tolerance * position_tolerance */
};

/* the three planes of a history of `pixels` pixels */
struct History {
    const Rec* a;
    const Rec* b;
    const Rec* c;
    size_t width;
    WPT_HD History(const Rec* planes, size_t w, size_t pixels) : a(planes), b(planes + pixels), c(planes + 2 * pixels), width(w) {}
    WPT_HD Rec guideA(int x, int y) const { return a[size_t(y) * width + size_t(x)]; }
    WPT_HD Rec guideB(int x, int y) const { return b[size_t(y) * width + size_t(x)]; }
    WPT_HD Rec colour(int x, int y) const { return c[size_t(y) * width + size_t(x)]; }
};

/* Pixel (x, y): guide B and the colour of the new history from the current frame's records (A, B, C of prepare(); guide A of
 * the new history is A itself) and the previous history.  `prev` NULL: the first frame.  `pixelOffset` (2 floats) and
 * `cameraOffset` (3 floats) are the pixel's offsets to the previous frame; both NULL: scene and camera at rest.
 * A tap is read guide first, its colour only if it counts; a tap of weight 0 is never read. */
WPT_HD void accumulatePixel(const Rec& A, const Rec& B, const Rec& C, uint32_t samplesSqrt, const History* prev, const float* pixelOffset,
        const float* cameraOffset, int x, int y, int width, int height, const Params& params, Rec& newB, Rec& newC)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int32_t m = wptdn::materialOf(A);
    float sw = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hv = 0.0f, hn = 0.0f;
    bool valid = false;
    if (prev) {
        /* where the history comes from: the taps (ix + i, iy + j) with the weights wy[j] * wx[i], and the point E as the
         * previous camera saw it */
        bool source = true;
        int ix = x, iy = y;
        float wx[2] = { 1.0f, 0.0f }, wy[2] = { 1.0f, 0.0f };
        Rec E = A;
        if (pixelOffset) {
            if (m < 0)
                source = false; /* the ground truth pass writes offset 0 where nothing was hit */
            else {
                const float fx = (float)x + pixelOffset[0];
                const float fy = (float)y + pixelOffset[1];
                if (!(fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height))
                    source = false; /* outside the frame, or NaN */
                else {
                    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
                    ix = (int)flx;
                    iy = (int)fly;
                    wx[1] = fx - flx;
                    wx[0] = 1.0f - wx[1];
                    wy[1] = fy - fly;
                    wy[0] = 1.0f - wy[1];
                    E.x = A.x + cameraOffset[0];
                    E.y = A.y + cameraOffset[1];
                    E.z = A.z + cameraOffset[2];
                }
            }
        }
        if (source)
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const float w = wy[j] * wx[i];
                    const int qx = ix + i, qy = iy + j;
                    if (w == 0.0f || qx < 0 || qy < 0 || qx >= width || qy >= height)
                        continue;
                    const Rec qA = prev->guideA(qx, qy);
                    if (wptdn::materialOf(qA) != m)
                        continue;
                    const Rec qB = prev->guideB(qx, qy);
                    if (m >= 0) {
                        if (!(wptdn::dot3(B, qB) >= params.normalCosMin))
                            continue;
                        Rec D;
                        D.x = qA.x - E.x;
                        D.y = qA.y - E.y;
                        D.z = qA.z - E.z;
                        D.w = 0.0f;
                        if (!(wptdn::dot3(D, D) <= params.tolerance2 * wptdn::dot3(E, E)))
                            continue;
                    }
                    const Rec qC = prev->colour(qx, qy);
                    sw += w;
                    hr += w * qC.x;
                    hg += w * qC.y;
                    hb += w * qC.z;
                    hv += w * qC.w;
                    hn += w * qB.w;
                    valid = true;
                }
    }
    newB = B;
    if (!valid) {
        /* reset, or the first frame; a pixel the frame did not sample starts at length 0: the next sampled frame replaces it */
        newC = C;
        newB.w = samplesSqrt == 0 ? 0.0f : 1.0f;
        return;
    }
    const float Hr = hr / sw, Hg = hg / sw, Hb = hb / sw, Hv = hv / sw, Hn = hn / sw;
    if (samplesSqrt == 0) {
        /* not sampled in this frame: the history is carried over */
        newC.x = Hr;
        newC.y = Hg;
        newC.z = Hb;
        newC.w = Hv;
        newB.w = Hn;
        return;
    }
    float N = Hn + 1.0f;
    if (!(N < params.maxHistory))
        N = params.maxHistory;
    const float a = 1.0f / N;
    const float b = 1.0f - a;
    newC.x = b * Hr + a * C.x;
    newC.y = b * Hg + a * C.y;
    newC.z = b * Hb + a * C.z;
    newC.w = (b * b) * Hv + (a * a) * C.w; /* the variance of a weighted mean of independent estimates */
    newB.w = N;
}

/* One frame into a history on the host, as the device runs it.  `prev` (may be NULL) and `out`: 3 * width * height records that
 * do not overlap; `pixelOffsets` (2 floats per pixel) and `cameraOffsets` (3) both NULL or both given; `lengthOut` may be NULL. */
inline void accumulateHost(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions, const float* normals,
        const int32_t* materials, const float* pixelOffsets, const float* cameraOffsets, const Rec* prev, uint32_t width, uint32_t height,
        const Params& params, Rec* out, float* lengthOut)
{
    const size_t pixels = size_t(width) * height;
    const History history(prev ? prev : out, width, pixels); /* never read without `prev` */
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const size_t p = size_t(y) * width + x;
            Rec A, B, C, newB, newC;
            wptdn::prepare(frame + 3 * p, moments + 3 * p, samplesSqrt[p], positions + 3 * p, normals + 3 * p, materials[p], A, B, C);
            accumulatePixel(A, B, C, samplesSqrt[p], prev ? &history : nullptr, pixelOffsets ? pixelOffsets + 2 * p : nullptr,
                    cameraOffsets ? cameraOffsets + 3 * p : nullptr, int(x), int(y), int(width), int(height), params, newB, newC);
            out[p] = A;
            out[pixels + p] = newB;
            out[2 * pixels + p] = newC;
            if (lengthOut)
                lengthOut[p] = newB.w;
        }
}

/* The filter's iterations on a history on the host, as the device runs them: iteration 1 reads the history's planes, later ones
 * alternate between the two planes of `scratch` (2 * width * height records; not read with no iterations); the history is never
 * written.  `variance` may be NULL.  No iterations: the accumulated frame and its variance. */
inline void denoiseHistoryHost(const Rec* history, uint32_t width, uint32_t height, const wptdn::Params& params, uint32_t iterations,
        Rec* scratch, float* out, float* variance)
{
    const size_t pixels = size_t(width) * height;
    const Rec* from = history + 2 * pixels;
    for (uint32_t i = 0; i < iterations; i++) {
        const wptdn::HostFetch fetch = { history, history + pixels, from, width };
        Rec* to = scratch + (i & 1u) * pixels;
        for (uint32_t y = 0; y < height; y++)
            for (uint32_t x = 0; x < width; x++)
                to[size_t(y) * width + x] = wptdn::filterPixel(fetch, int(x), int(y), int(width), int(height), 1 << i, params);
        from = to;
    }
    for (size_t p = 0; p < pixels; p++) {
        out[3 * p] = from[p].x;
        out[3 * p + 1] = from[p].y;
        out[3 * p + 2] = from[p].z;
        if (variance)
            variance[p] = from[p].w;
    }
}

} /* namespace wpttm */

#endif
