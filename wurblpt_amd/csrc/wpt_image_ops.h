/*
 * wpt_image_ops.h -- the image operations of the output side's second half (postproc.hpp:112-309): bilinear resampling
 * (scale), the warp of a frame through a lens model (applyLensDistortion / distort / undistort), the firefly filter
 * (despeckle), and measured distances turned into coordinates (cameraSpaceDistanceToCoords, cameraSpaceToPMDSpace as a flag).
 * Restated in float, operation for operation, every product and sum rounded on its own (-ffp-contract=off), so that the
 * device, the host and the reference's functions give the same bits.
 *
 * Images are [height][width][c] floats, row 0 at the bottom.
 *
 * The sampling rule (texture_image.hpp:182-212, float data, no sRGB) is shared by resample, warp and coordinates:
 *   uv = tc - floor(tc), so coordinates outside [0, 1) wrap;
 *   uvs = max(0, uv.s * W - 0.5f), x0 = (size_t)uvs, x1 = x0 + 1 clamped to W - 1, alpha = uvs - x0; the same for t;
 *   mix(mix(v00, v10, alpha), mix(v01, v11, alpha), beta) with mix(x, y, a) = x + a * (y - x).
 * A texel is expanded by the image's component count before it is mixed (texture_image.hpp:152-177): 3 components give
 * (r, g, b, 1), 4 pass through, 1 gives (v, v, v, 1) and 2 give (v0, v0, v0, v1).  Output component c is component c of that
 * expansion, so OUTPUT COMPONENT 1 OF A TWO-COMPONENT IMAGE IS COMPONENT 0's VALUE, not component 1's: that is what the
 * reference's functions return, and it is kept.
 * A sampling coordinate that is not finite is undefined in the reference (it asserts); here every component of that output
 * pixel is +0, on the host and on the device.
 *
 * Written once; compiled for the device (wpt_k_image_ops.hip), for the host (wpt_postproc_*_host in wpt_capi_postproc.hip) and, outside
 * the library and without a header of HIP, by tests/image_ops_check.cpp.
 */
#ifndef WPT_IMAGE_OPS_H
#define WPT_IMAGE_OPS_H

#include <stddef.h>
#include <stdint.h>

#include "wpt_lens.h"
#include "wpt_math.h"
#include "wpt_postproc.h"

namespace wptio {

enum : uint32_t {
    SIDE_MAX = 65535u,    /* width and height: a pixel's coordinates convert to float exactly and stay far inside 32 bits */
    COMPONENTS_MAX = 4u
};

/* an image in memory (the device's or the host's) */
struct Image {
    const float* data;
    uint32_t width, height, comps;
};

WPT_HD bool isFinite(float v)
{
    return (wptm::float_to_bits(v) & 0x7f800000u) != 0x7f800000u;
}

/* gvm.hpp:166 */
WPT_HD float mix(float x, float y, float alpha)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return x + alpha * (y - x);
}

/* The first `n` components of Texture::value at finite texture coordinates (s, t); n <= img.comps. */
WPT_HD void sample(const Image& img, float s, float t, float* out, uint32_t n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = s - __builtin_floorf(s);
    const float v = t - __builtin_floorf(t);
    const float us = u * (float)img.width - 0.5f;
    const float vt = v * (float)img.height - 0.5f;
    const float uvs = us > 0.0f ? us : 0.0f;
    const float uvt = vt > 0.0f ? vt : 0.0f;
    size_t x0 = (size_t)uvs;
    size_t y0 = (size_t)uvt;
    const float alpha = uvs - (float)x0;
    const float beta = uvt - (float)y0;
    size_t x1 = x0 + 1;
    size_t y1 = y0 + 1;
    /* value(x, y) clamps every index at the far edge (texture_image.hpp:87-90); u = 1 after rounding lands there */
    const size_t xMax = img.width - 1, yMax = img.height - 1;
    x0 = x0 > xMax ? xMax : x0;
    x1 = x1 > xMax ? xMax : x1;
    y0 = y0 > yMax ? yMax : y0;
    y1 = y1 > yMax ? yMax : y1;
    const size_t comps = img.comps;
    const float* p00 = img.data + (y0 * img.width + x0) * comps;
    const float* p10 = img.data + (y0 * img.width + x1) * comps;
    const float* p01 = img.data + (y1 * img.width + x0) * comps;
    const float* p11 = img.data + (y1 * img.width + x1) * comps;
    for (uint32_t c = 0; c < n; c++) {
        const uint32_t k = comps == 2 ? 0u : c; /* the expansion's component c */
        const float a = mix(p00[k], p10[k], alpha);
        const float b = mix(p01[k], p11[k], alpha);
        out[c] = mix(a, b, beta);
    }
}

/* sample(), or zeros where a coordinate is not finite */
WPT_HD void sampleOrZero(const Image& img, float s, float t, float* out, uint32_t n)
{
    if (isFinite(s) && isFinite(t)) {
        sample(img, s, t, out, n);
    } else {
        for (uint32_t c = 0; c < n; c++)
            out[c] = 0.0f;
    }
}

/* scale(), postproc.hpp:112-136: pixel (x, y) of the newWidth x newHeight image, img.comps floats */
WPT_HD void resamplePixel(const Image& img, uint32_t x, uint32_t y, uint32_t newWidth, uint32_t newHeight, float* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float tcx = ((float)x + 0.5f) / (float)newWidth;
    const float tcy = ((float)y + 0.5f) / (float)newHeight;
    sampleOrZero(img, tcx, tcy, out, img.comps);
}

/* applyLensDistortion(), postproc.hpp:197-236: pixel (x, y) of the warped image, img.comps floats.  forward: the image is an
 * undistorted render and the output what the lens makes of it, so the output pixel is looked up at its undistorted place. */
WPT_HD void warpPixel(const Image& img, const wptlens::Coeffs& lens, bool forward, uint32_t x, uint32_t y, float* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float invWidth = 1.0f / (float)img.width;
    const float invHeight = 1.0f / (float)img.height;
    float p = ((float)x + 0.5f) * invWidth;
    float q = ((float)y + 0.5f) * invHeight;
    if (forward) {
        const wptlens::Point r = wptlens::undistortCall(lens, p, q, img.width, img.height);
        p = r.p;
        q = r.q;
    } else {
        wptlens::distort(lens, p, q);
    }
    sampleOrZero(img, p, q, out, img.comps);
}

/* cameraSpaceDistanceToCoords(), postproc.hpp:252-287, and with pmdSpace cameraSpaceToPMDSpace() (:289-309) behind it: three
 * floats of pixel (x, y).  The distance is component 0 of `img` where the lens puts the pixel. */
WPT_HD void coordsPixel(const Image& img, const wptlens::Coeffs& lens, bool pmdSpace, uint32_t x, uint32_t y, float* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float invWidth = 1.0f / (float)img.width;
    const float invHeight = 1.0f / (float)img.height;
    const float p = ((float)x + 0.5f) * invWidth;
    const float q = ((float)y + 0.5f) * invHeight;
    float dp = p, dq = q;
    wptlens::distort(lens, dp, dq);
    if (!(isFinite(dp) && isFinite(dq))) {
        out[0] = out[1] = out[2] = 0.0f;
        return;
    }
    float distance;
    sample(img, dp, dq, &distance, 1);
    const float ux = (p - lens.cx) * lens.ifx;
    const float uy = (q - lens.cy) * lens.ify;
    const float length = __builtin_sqrtf((ux * ux + uy * uy) + 1.0f); /* gvm.hpp:1183-1194 */
    const float X = (ux / length) * distance;                           /* normalize() divides (gvm.hpp:1201-1204) */
    const float Y = (uy / length) * distance;
    const float Z = (1.0f / length) * distance;
    out[0] = X;
    out[1] = pmdSpace ? -Y : Y;
    out[2] = pmdSpace ? Z : -Z;
}

/* despeckle(), postproc.hpp:143-193: RGB of pixel (x, y).  Fetch: rgb(xx, yy, v) gives the pixel at the coordinates clamped to
 * the frame; xx, yy lie at most one outside.  std::sort of nine elements is libstdc++'s insertion sort, which keeps equal
 * luminances in the neighbourhood's row-major order; the same order follows from ranks without a sort or a branch:
 * rank(i) = the number of j with lum_j < lum_i, or lum_j == lum_i and j < i.  The inputs must be finite. */
template<class Fetch> WPT_HD void despecklePixel(const Fetch& fetch, int x, int y, float minFactor, float* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float rgb[9][3];
    float lum[9];
    for (int r = -1; r <= 1; r++)
        for (int c = -1; c <= 1; c++) {
            const int i = (r + 1) * 3 + c + 1;
            fetch.rgb(x + c, y + r, rgb[i]);
            wptpp::V3 v;
            v.x = rgb[i][0];
            v.y = rgb[i][1];
            v.z = rgb[i][2];
            lum[i] = wptpp::rgbToXyz(v).y;
        }
    float median[3] = { 0.0f, 0.0f, 0.0f };
    float lum7 = 0.0f, lum8 = 0.0f;
    for (int i = 0; i < 9; i++) {
        int rank = 0;
        for (int j = 0; j < 9; j++)
            rank += (lum[j] < lum[i] || (lum[j] == lum[i] && j < i)) ? 1 : 0;
        median[0] = rank == 4 ? rgb[i][0] : median[0];
        median[1] = rank == 4 ? rgb[i][1] : median[1];
        median[2] = rank == 4 ? rgb[i][2] : median[2];
        lum7 = rank == 7 ? lum[i] : lum7;
        lum8 = rank == 8 ? lum[i] : lum8;
    }
    const bool speckle = lum[4] >= lum8 && lum[4] >= minFactor * lum7;
    out[0] = speckle ? median[0] : rgb[4][0];
    out[1] = speckle ? median[1] : rgb[4][1];
    out[2] = speckle ? median[2] : rgb[4][2];
}

/* a frame in memory, coordinates clamped per fetch */
struct ClampFetch {
    const float* data;
    int width, height;
    WPT_HD void rgb(int xx, int yy, float* v) const
    {
        xx = xx < 0 ? 0 : (xx > width - 1 ? width - 1 : xx);
        yy = yy < 0 ? 0 : (yy > height - 1 ? height - 1 : yy);
        const float* p = data + (size_t(yy) * size_t(width) + size_t(xx)) * 3;
        v[0] = p[0];
        v[1] = p[1];
        v[2] = p[2];
    }
};

/* ---- the host loops: what the device runs with one lane per output pixel ---- */

inline void resampleHost(const Image& img, uint32_t newWidth, uint32_t newHeight, float* out)
{
    for (uint32_t y = 0; y < newHeight; y++)
        for (uint32_t x = 0; x < newWidth; x++)
            resamplePixel(img, x, y, newWidth, newHeight, out + (size_t(y) * newWidth + x) * img.comps);
}

inline void warpHost(const Image& img, const wptlens::Coeffs& lens, bool forward, float* out)
{
    for (uint32_t y = 0; y < img.height; y++)
        for (uint32_t x = 0; x < img.width; x++)
            warpPixel(img, lens, forward, x, y, out + (size_t(y) * img.width + x) * img.comps);
}

inline void despeckleHost(const float* rgb, uint32_t width, uint32_t height, float minFactor, float* out)
{
    const ClampFetch fetch = { rgb, int(width), int(height) };
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++)
            despecklePixel(fetch, int(x), int(y), minFactor, out + (size_t(y) * width + x) * 3);
}

inline void coordsHost(const Image& img, const wptlens::Coeffs& lens, bool pmdSpace, float* out)
{
    for (uint32_t y = 0; y < img.height; y++)
        for (uint32_t x = 0; x < img.width; x++)
            coordsPixel(img, lens, pmdSpace, x, y, out + (size_t(y) * img.width + x) * 3);
}

} /* namespace wptio */

#endif
