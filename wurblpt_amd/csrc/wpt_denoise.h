/*
 * wpt_denoise.h -- the spatial denoiser of a rendered frame: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) whose
 * colour weight is guided by the frame's own variance estimate (Schied et al. 2017, spatial part only).  Restated in float,
 * operation for operation, every product and sum rounded on its own (-ffp-contract=off), so that the device and the host give
 * the same bits.  DESIGN.md, "Denoiser", holds the formula.
 *
 * Per pixel the filter reads three 16-byte records:
 *   guide A = P.xyz (camera space position of the first hit) and the bits of m (material index, -1 = nothing hit)
 *   guide B = n.xyz (camera space material normal)
 *   colour  = rgb and V, the variance of the luminance
 * prepare() makes them from the render's outputs (prepareDemodulated() with the surface's own colours taken out, which
 * finishDemodulated() puts back), filterPixel() is one pixel of one iteration; `Fetch` says where the records
 * of a pixel lie (device memory, a workgroup's tile in LDS, host arrays).
 * Written once; compiled for the device (wpt_k_denoise.hip), for the host (wpt_postproc_denoise_host) and, outside the library
 * and without a header of HIP, by tests/denoise_check.cpp.
 */
#ifndef WPT_DENOISE_H
#define WPT_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "wpt_math.h"

namespace wptdn {

enum : uint32_t {
    ITERATIONS_MAX = 8u,   /* steps 1 .. 128 */
    NORMAL_LOG2_MAX = 16u, /* the normal weight is at most c^65536 */
    SIDE_MAX = 65535u      /* width and height; a tap's coordinates stay far inside 32 bits */
};

/* wpt_denoise_params with the sigmas' squares and products taken once */
struct Params {
    float sigmaL;
    float sigmaZ2; /* sigma_z * sigma_z */
    uint32_t normalLog2;
};

/* a 16-byte record */
struct alignas(16) Rec {
    float x, y, z, w;
};

/* the Y row of wptpp::rgbToXyz (wpt_postproc.h) without the factor 100 */
constexpr float k_yr = 0.212671f, k_yg = 0.715160f, k_yb = 0.072169f;

WPT_HD float luminance(float r, float g, float b)
{
    return (k_yr * r + k_yg * g) + k_yb * b;
}

WPT_HD float dot3(const Rec& a, const Rec& b)
{
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

/* a channel's variance of the mean: the moment film's second moment minus the mean's square over N - 1; a pixel with fewer
 * than two samples has no estimate, and its standard deviation is taken to be its value */
WPT_HD float channelVariance(float frame, float moment, uint32_t samplesSqrt)
{
    if (samplesSqrt < 2)
        return frame * frame;
    const uint32_t N = samplesSqrt * samplesSqrt;
    const float d = moment - frame * frame;
    return (d > 0.0f ? d : 0.0f) / (float)(N - 1);
}

/* the three records of a pixel from what the render and the ground truth pass wrote for it; the channels count as fully
 * correlated: sigma_Y is the luminance of their standard deviations */
WPT_HD void prepare(const float* frame, const float* moments, uint32_t samplesSqrt, const float* position, const float* normal,
        int32_t material, Rec& guideA, Rec& guideB, Rec& colour)
{
    const float vr = channelVariance(frame[0], moments[0], samplesSqrt);
    const float vg = channelVariance(frame[1], moments[1], samplesSqrt);
    const float vb = channelVariance(frame[2], moments[2], samplesSqrt);
    const float sigmaY = luminance(__builtin_sqrtf(vr), __builtin_sqrtf(vg), __builtin_sqrtf(vb));
    guideA.x = position[0];
    guideA.y = position[1];
    guideA.z = position[2];
    guideA.w = wptm::bits_to_float((uint32_t)material);
    guideB.x = normal[0];
    guideB.y = normal[1];
    guideB.z = normal[2];
    guideB.w = 0.0f;
    colour.x = frame[0];
    colour.y = frame[1];
    colour.z = frame[2];
    colour.w = sigmaY * sigmaY;
}

/* ---- the demodulated form: the filter runs on (frame - emission) / albedo, the light that arrives at the first hit, and the
 * surface's own colours are put back afterwards, so that a texture is not filtered with the noise.  `albedo` and `emission`
 * are the planes of the first-hit colour pass (wpt_first_hit_colours*). ---- */
constexpr float k_albedoFloorDefault = 1.0f / 64;

/* what a channel is divided by: its albedo, or 1 where the albedo lies below the floor (a dark texel would blow the noise up) */
WPT_HD float demodulationDivisor(float albedo, float albedoFloor)
{
    return albedo >= albedoFloor ? albedo : 1.0f;
}

/* prepare() for the demodulated form: u = (frame - emission) / d per channel, its variance is the channel's over d * d; a pixel
 * with fewer than two samples has no estimate, and its standard deviation is taken to be |u|.  u may be negative where a lamp
 * covers the pixel's centre but not all of its footprint. */
WPT_HD void prepareDemodulated(const float* frame, const float* moments, uint32_t samplesSqrt, const float* position, const float* normal,
        int32_t material, const float* albedo, const float* emission, float albedoFloor, Rec& guideA, Rec& guideB, Rec& colour)
{
    float u[3], v[3];
    for (int c = 0; c < 3; c++) {
        const float d = demodulationDivisor(albedo[c], albedoFloor);
        u[c] = (frame[c] - emission[c]) / d;
        v[c] = samplesSqrt >= 2 ? channelVariance(frame[c], moments[c], samplesSqrt) / (d * d) : u[c] * u[c];
    }
    const float sigmaY = luminance(__builtin_sqrtf(v[0]), __builtin_sqrtf(v[1]), __builtin_sqrtf(v[2]));
    guideA.x = position[0];
    guideA.y = position[1];
    guideA.z = position[2];
    guideA.w = wptm::bits_to_float((uint32_t)material);
    guideB.x = normal[0];
    guideB.y = normal[1];
    guideB.z = normal[2];
    guideB.w = 0.0f;
    colour.x = u[0];
    colour.y = u[1];
    colour.z = u[2];
    colour.w = sigmaY * sigmaY;
}

/* the filtered record back to radiance: out = c * d + emission per channel.  The record's w, the variance of the DEMODULATED
 * luminance, is not converted. */
WPT_HD void finishDemodulated(const Rec& colour, const float* albedo, const float* emission, float albedoFloor, float* out)
{
    out[0] = colour.x * demodulationDivisor(albedo[0], albedoFloor) + emission[0];
    out[1] = colour.y * demodulationDivisor(albedo[1], albedoFloor) + emission[1];
    out[2] = colour.z * demodulationDivisor(albedo[2], albedoFloor) + emission[2];
}

WPT_HD int32_t materialOf(const Rec& guideA)
{
    return (int32_t)wptm::float_to_bits(guideA.w);
}

/* the weights of the B3 spline's taps -2 .. 2: (1, 4, 6, 4, 1) / 16 */
WPT_HD float b3(int d)
{
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

/* Pixel (x, y) of iteration `step` = 2^i of a width x height frame: the filtered colour and the variance of its luminance.
 * Fetch: guideA(x, y), guideB(x, y), colour(x, y) of a pixel inside the frame.  Taps outside the frame are skipped, as are
 * taps on another material; the centre tap has the weight 9/64 whatever the guide holds, so the sum of weights is positive. */
template<class Fetch> WPT_HD Rec filterPixel(const Fetch& fetch, int x, int y, int width, int height, int step, const Params& params)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    /* g: the (1,2,1) x (1,2,1) mean of the variance around the pixel, over the taps inside the frame */
    float gSum = 0.0f, gWeights = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height)
                continue;
            const float k = (float)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            gSum += k * fetch.colour(qx, qy).w;
            gWeights += k;
        }
    const float g = gSum / gWeights;
    const float L = params.sigmaL * __builtin_sqrtf(g) + 1e-10f;

    const Rec pA = fetch.guideA(x, y);
    const Rec pB = fetch.guideB(x, y);
    const Rec pC = fetch.colour(x, y);
    const int32_t pMaterial = materialOf(pA);
    const float pY = luminance(pC.x, pC.y, pC.z);

    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx, qy = y + step * dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height)
                continue;
            float w = b3(dy) * b3(dx);
            Rec qC = pC;
            if (dx != 0 || dy != 0) {
                const Rec qA = fetch.guideA(qx, qy);
                if (materialOf(qA) != pMaterial)
                    continue;
                qC = fetch.colour(qx, qy);
                float wn = 1.0f, ez = 0.0f;
                if (pMaterial >= 0) {
                    const Rec qB = fetch.guideB(qx, qy);
                    const float c = dot3(pB, qB);
                    wn = c > 0.0f ? c : 0.0f;
                    for (uint32_t k = 0; k < params.normalLog2; k++)
                        wn = wn * wn;
                    Rec D;
                    D.x = qA.x - pA.x;
                    D.y = qA.y - pA.y;
                    D.z = qA.z - pA.z;
                    D.w = 0.0f;
                    const float t = dot3(pB, D);
                    const float dd = dot3(D, D);
                    ez = dd == 0.0f ? 0.0f : (t * t) / (params.sigmaZ2 * dd);
                }
                const float el = __builtin_fabsf(luminance(qC.x, qC.y, qC.z) - pY) / L;
                w = w * wn * wptm::expf_(-(ez + el));
            }
            sw += w;
            sr += w * qC.x;
            sg += w * qC.y;
            sb += w * qC.z;
            sv += (w * w) * qC.w;
        }
    Rec out;
    out.x = sr / sw;
    out.y = sg / sw;
    out.z = sb / sw;
    out.w = sv / (sw * sw);
    return out;
}

/* where the host keeps a frame's records */
struct HostFetch {
    const Rec* a;
    const Rec* b;
    const Rec* c;
    size_t width;
    const Rec& guideA(int x, int y) const { return a[size_t(y) * width + size_t(x)]; }
    const Rec& guideB(int x, int y) const { return b[size_t(y) * width + size_t(x)]; }
    const Rec& colour(int x, int y) const { return c[size_t(y) * width + size_t(x)]; }
};

/* the iterations on the host: steps 1, 2, 4, ... over the two colour buffers; returns the buffer that holds the result */
inline Rec* iterateHost(const Rec* a, const Rec* b, Rec* from, Rec* to, uint32_t width, uint32_t height, const Params& params, uint32_t iterations)
{
    for (uint32_t i = 0; i < iterations; i++) {
        const HostFetch fetch = { a, b, from, width };
        for (uint32_t y = 0; y < height; y++)
            for (uint32_t x = 0; x < width; x++)
                to[size_t(y) * width + x] = filterPixel(fetch, int(x), int(y), int(width), int(height), 1 << i, params);
        Rec* t = from;
        from = to;
        to = t;
    }
    return from;
}

/* The whole filter on the host, as the device runs it.  `scratch`: 4 * width * height records (64 bytes per pixel: the two
 * guides and the two colour buffers the iterations alternate between).  `variance` may be NULL. */
inline void denoiseHost(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions, const float* normals,
        const int32_t* materials, uint32_t width, uint32_t height, const Params& params, uint32_t iterations, Rec* scratch, float* out,
        float* variance)
{
    const size_t pixels = size_t(width) * height;
    Rec* a = scratch;
    Rec* b = scratch + pixels;
    Rec* from = scratch + 2 * pixels;
    for (size_t p = 0; p < pixels; p++)
        prepare(frame + 3 * p, moments + 3 * p, samplesSqrt[p], positions + 3 * p, normals + 3 * p, materials[p], a[p], b[p], from[p]);
    from = iterateHost(a, b, from, scratch + 3 * pixels, width, height, params, iterations);
    for (size_t p = 0; p < pixels; p++) {
        out[3 * p] = from[p].x;
        out[3 * p + 1] = from[p].y;
        out[3 * p + 2] = from[p].z;
        if (variance)
            variance[p] = from[p].w;
    }
}

/* The demodulated form on the host, as the device runs it: the same scratch, the same iterations.  `variance` (may be NULL)
 * receives the variance of the demodulated luminance. */
inline void denoiseDemodulatedHost(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions,
        const float* normals, const int32_t* materials, const float* albedo, const float* emission, uint32_t width, uint32_t height,
        const Params& params, uint32_t iterations, float albedoFloor, Rec* scratch, float* out, float* variance)
{
    const size_t pixels = size_t(width) * height;
    Rec* a = scratch;
    Rec* b = scratch + pixels;
    Rec* from = scratch + 2 * pixels;
    for (size_t p = 0; p < pixels; p++)
        prepareDemodulated(frame + 3 * p, moments + 3 * p, samplesSqrt[p], positions + 3 * p, normals + 3 * p, materials[p], albedo + 3 * p,
                emission + 3 * p, albedoFloor, a[p], b[p], from[p]);
    from = iterateHost(a, b, from, scratch + 3 * pixels, width, height, params, iterations);
    for (size_t p = 0; p < pixels; p++) {
        finishDemodulated(from[p], albedo + 3 * p, emission + 3 * p, albedoFloor, out + 3 * p);
        if (variance)
            variance[p] = from[p].w;
    }
}

} /* namespace wptdn */

#endif
