/*
 * wpt_shutter.h -- the rolling shutter's rule, once: which exposure interval a frame row has.  The moving-scene kernels
 * (wpt_blocks.h, blockNewFrom) and the host functions behind wpt_shutter_row_interval / wpt_shutter_span (wpt_capi_render.hip)
 * compile this text, so a row's interval on the device is the one the host reports, bit for bit.  No HIP call, no header of the
 * path tracer.
 *
 * A frame of `height` rows (row 0 = bottom, as everywhere) is read out row by row, one row every `rowTime`, from the top row
 * down (fromTop) or from the bottom row up.  With k the row's place in that order,
 *
 *     s = (float)k * rowTime      a = t0 + s      b = t1 + s
 *
 * each operation rounded once (the units that include this are built with -ffp-contract=off), and the row is exposed over
 * [a, b] as a global-shutter frame is over [t0, t1].  height <= 65535, so (float)k is exact; a and b are monotone in k.
 */
#ifndef WPT_SHUTTER_H
#define WPT_SHUTTER_H

#include <stdint.h>

#if defined(__HIPCC__)
#define WPT_SHUTTER_HD __host__ __device__ inline
#else
#define WPT_SHUTTER_HD inline
#endif

namespace wptshutter {

/* a launch's shutter as the kernels carry it; { 0.0f, 0 }: none, every row has [t0, t1] */
struct Rows {
    float rowTime;
    uint32_t fromTop;
};

struct Interval {
    float a, b;
};

/* the place of frame row y in the readout order */
WPT_SHUTTER_HD uint32_t readoutIndex(uint32_t fromTop, uint32_t height, uint32_t y)
{
    return fromTop ? height - 1u - y : y;
}

/* the exposure interval of frame row y */
WPT_SHUTTER_HD Interval rowInterval(Rows rows, float t0, float t1, uint32_t height, uint32_t y)
{
    const float s = (float)readoutIndex(rows.fromTop, height, y) * rows.rowTime;
    Interval iv;
    iv.a = t0 + s;
    iv.b = t1 + s;
    return iv;
}

/* Host: NULL for a shutter the library renders with over a frame of `height` rows exposed over [t0, t1], or why not.  The
 * row read last must still have a finite interval; rows before it then have one too. */
inline const char* refusal(float rowTime, uint32_t fromTop, uint32_t reserved0, uint32_t reserved1, float t0, float t1, uint32_t height)
{
    const float fmax = 3.40282346638528859812e+38f;
    if (!(rowTime >= 0.0f && rowTime <= fmax)) /* (false for a NaN) */
        return "shutter: row_time must be finite and >= 0";
    if (fromTop > 1u)
        return "shutter: from_top must be 0 or 1";
    if (reserved0 != 0u || reserved1 != 0u)
        return "shutter: the reserved words must be 0";
    if (height == 0u || height > 65535u)
        return "shutter: height must lie in 1 .. 65535";
    const Rows rows = { rowTime, 0u };
    const Interval last = rowInterval(rows, t0, t1, height, height - 1u);
    if (!(last.a >= -fmax && last.a <= fmax && last.b >= -fmax && last.b <= fmax))
        return "shutter: the readout overflows, the interval of the row read last is not finite";
    return nullptr;
}

} /* namespace wptshutter */

#endif
