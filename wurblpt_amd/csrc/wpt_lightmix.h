/*
 * wpt_lightmix.h -- light groups after the render: the check of a launch's group table and the mix of planes into one frame,
 *   out[p][c] = (((0 + w[0][c] * P0[p][c]) + w[1][c] * P1[p][c]) + ...)     in float, planes in order,
 * every product and every sum rounded on its own (no fused multiply-add), so that the device and the host give the same bits.
 * The weights are an RGB triple per plane: a group's intensity and colour, chosen after the render.  The planes may be a
 * light-groups launch's or the transient film's.
 * Written once; compiled for the device (wpt_lightmix_kernel in wpt_capi_postproc.hip), for the host (wpt_postproc_mix_planes_host) and,
 * outside the library and without a header of HIP, by tests/lightmix_check.cpp.
 */
#ifndef WPT_LIGHTMIX_H
#define WPT_LIGHTMIX_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WPT_MIX_HD __host__ __device__ __forceinline__
#else
#define WPT_MIX_HD inline
#endif

namespace wptmix {

enum : uint32_t {
    GROUPS_MAX = 255u,  /* WPT_LIGHT_GROUPS_MAX */
    GROUP_NONE = 0xffu, /* WPT_LIGHT_GROUP_NONE: the emitter's light reaches the frame only */
    PLANES_MAX = 4096u  /* planes one mix takes: the transient film's WPT_TRANSIENT_MAX_BINS */
};

/* what a group table is refused for; TABLE_ENTRY: `at` is the material whose group is neither below the count nor NONE */
enum TableError { TABLE_OK = 0, TABLE_NULL, TABLE_GROUP_COUNT, TABLE_ENTRY, TABLE_ENV_GROUP };

/* the check of a launch's table: `groupOfMaterial` holds `materialCount` bytes, each a group below `groupCount` or GROUP_NONE,
 * and so is `envGroup`.  Reads nothing when the count is out of range. */
inline TableError checkTable(const uint8_t* groupOfMaterial, uint32_t materialCount, uint32_t groupCount, uint32_t envGroup, uint32_t* at)
{
    if (at)
        *at = 0;
    if (!groupOfMaterial)
        return TABLE_NULL;
    if (groupCount == 0 || groupCount > GROUPS_MAX)
        return TABLE_GROUP_COUNT;
    for (uint32_t m = 0; m < materialCount; m++)
        if (groupOfMaterial[m] >= groupCount && groupOfMaterial[m] != GROUP_NONE) {
            if (at)
                *at = m;
            return TABLE_ENTRY;
        }
    if (envGroup >= groupCount && envGroup != GROUP_NONE)
        return TABLE_ENV_GROUP;
    return TABLE_OK;
}

/* value `i` (pixel i / 3, channel i % 3) of the mix of `planeCount` planes that lie `stride` floats apart */
WPT_MIX_HD float mixValue(const float* planes, uint32_t planeCount, size_t stride, const float* weights, size_t i)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float* w = weights + i % 3;
    const float* p = planes + i;
    float sum = 0.0f;
    for (uint32_t k = 0; k < planeCount; k++) {
        const float term = w[3 * size_t(k)] * p[size_t(k) * stride];
        sum = sum + term;
    }
    return sum;
}

/* the whole mix on the host, value by value */
inline void mixHost(const float* planes, uint32_t planeCount, size_t stride, uint64_t pixels, const float* weights, float* out)
{
    for (uint64_t i = 0; i < pixels * 3; i++)
        out[i] = mixValue(planes, planeCount, stride, weights, size_t(i));
}

} /* namespace wptmix */

#endif
