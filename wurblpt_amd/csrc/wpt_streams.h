/*
 * wpt_streams.h -- sample streams after the render: the mean of K stream frames, the stream moment film, the merge of two such
 * results, and the plan that splits a frame's samples into streams.
 *   mean[i]   = (((P0[i] + P1[i]) + P2[i]) + ...) * (1 / (float)K)                planes in order
 *   moment[i] = (((P0[i] * P0[i] + P1[i] * P1[i]) + P2[i] * P2[i]) + ...) * (1 / (float)K)
 *   merge[i]  = ((float)Ka * a[i] + (float)Kb * b[i]) / (float)(Ka + Kb)
 * in float, every product, sum and quotient rounded on its own (no fused multiply-add), so that the device and the host give the
 * same bits -- except where a result is NaN: there both give a NaN, but its sign and payload are the implementation's (inf - inf
 * is a negative NaN on x86 and a positive one on the GPU).  With K = 1 the mean is the plane (x * 1.0f) and the moment its
 * square.  With N = K the moment film is what the
 * variance formula of the adaptive film expects, (moment - mean^2) * N / (N - 1) / N: the variance of the pixel's mean from K
 * independent stream means, unbiased whatever the strata within a stream.
 * Written once; compiled for the device (wpt_k_streams.hip), for the host (wpt_postproc_mean_planes_host and _merge_means_host in
 * wpt_capi_postproc.hip, wpt_split_plan in wpt_capi.hip) and, outside the library and without a header of HIP, by tests/streams_check.cpp.
 */
#ifndef WPT_STREAMS_H
#define WPT_STREAMS_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WPT_STREAMS_HD __host__ __device__ __forceinline__
#else
#define WPT_STREAMS_HD inline
#endif

namespace wptstr {

/* a frame should cover this many pixels per lane of the device before its samples stay one stream (splitPlan) */
enum : uint32_t { SPLIT_PIXELS_PER_LANE = 4u };

/* value `i` of the mean of `planeCount` >= 1 planes that lie `stride` floats apart; *moment (or NULL): the mean of their squares */
WPT_STREAMS_HD float meanValue(const float* planes, uint32_t planeCount, size_t stride, size_t i, float* moment)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float* p = planes + i;
    float sum = p[0];
    float squares = p[0] * p[0];
    for (uint32_t k = 1; k < planeCount; k++) {
        const float v = p[size_t(k) * stride];
        const float square = v * v;
        sum = sum + v;
        squares = squares + square;
    }
    const float inv = 1.0f / float(planeCount);
    if (moment)
        *moment = squares * inv;
    return sum * inv;
}

/* one value of the merge of a mean (or moment) over countA streams with one over countB other streams; countA + countB > 0 */
WPT_STREAMS_HD float mergeValue(float a, uint32_t countA, float b, uint32_t countB)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float wa = float(countA) * a;
    const float wb = float(countB) * b;
    const float sum = wa + wb;
    return sum / float(uint64_t(countA) + uint64_t(countB));
}

/* the whole mean and merge on the host, value by value */
inline void meanHost(const float* planes, uint32_t planeCount, size_t stride, uint64_t values, float* mean, float* moment)
{
    for (uint64_t i = 0; i < values; i++)
        mean[i] = meanValue(planes, planeCount, stride, size_t(i), moment ? moment + i : nullptr);
}

inline void mergeHost(const float* a, uint32_t countA, const float* b, uint32_t countB, uint64_t values, float* out)
{
    for (uint64_t i = 0; i < values; i++)
        out[i] = mergeValue(a[i], countA, b[i], countB);
}

/* How a frame of `pixels` pixels with samplesSqrt^2 samples each is split for a device that holds `lanes` lanes: K = k^2 streams
 * of (samplesSqrt / k)^2 samples, k a divisor of samplesSqrt that leaves a stream at least 2 x 2 strata (or k = 1).  Among these
 * k in increasing order the first with k^2 * pixels >= SPLIT_PIXELS_PER_LANE * lanes, otherwise the largest.  The total sample
 * count is kept exactly and K is a square.  False: an argument is 0. */
inline bool splitPlan(uint64_t pixels, uint32_t samplesSqrt, uint32_t lanes, uint32_t* streamCount, uint32_t* streamSamplesSqrt)
{
    if (pixels == 0 || samplesSqrt == 0 || lanes == 0)
        return false;
    uint32_t best = 1;
    /* (k below 2^16: K is 32 bits) */
    for (uint32_t k = 1; k <= samplesSqrt / 2 && k <= 0xffffu; k++) {
        if (samplesSqrt % k != 0)
            continue;
        best = k;
        /* (a product beyond 2^64 is enough in any case) */
        const uint64_t k2 = uint64_t(k) * k;
        if (pixels > UINT64_MAX / k2 || k2 * pixels >= uint64_t(SPLIT_PIXELS_PER_LANE) * lanes)
            break;
    }
    /* (k = 1 is the only candidate for samplesSqrt below 4 and for a prime) */
    *streamCount = best * best;
    *streamSamplesSqrt = samplesSqrt / best;
    return true;
}

} /* namespace wptstr */

#endif
