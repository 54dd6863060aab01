/*
 * wpt_tof.h -- the accumulate rule of the amplitude-modulated continuous-wave time-of-flight sensor
 * (SensorTofAmcw::accumulateRadiance, sensor_tof_amcw.hpp:227-252), restated operation for operation in float.
 * Written once; compiled for the device (FEAT_TOF kernels, wpt_blocks.h) and for the host (wpt_tof_accumulate_host in
 * wpt_capi_sensors.hip, which the tests hold against the formula).  Needs -ffp-contract=off like everything here.
 *
 * A contribution of radiance.w (the near infrared channel) with the optical path length opl.w adds to a pixel's taps
 *   energy = radiance.w * 1000 * pixelArea * 0.5 * exposureTime          (left to right)
 *   t      = contrast * cos(tau + 2 pi * opl.w * fracModfreqC)           for light from a ToF light, 0 for any other
 *   a += 0.5 * energy * (1 + t),  b += 0.5 * energy * (1 - t),  total += energy
 * No gate applies.  The cosine is wpt_math.h's, which is glibc's bit for bit.
 */
#ifndef WPT_TOF_H
#define WPT_TOF_H

#include "wpt_math.h"

namespace wpttof {

/* the sensor's constants as the kernels read them: one float array in device memory (BinsView::edges in FEAT_TOF kernels) */
enum { C_PIXEL_AREA = 0, C_EXPOSURE_TIME = 1, C_CONTRAST = 2, C_FRAC_MODFREQ_C = 3, C_TAU = 4 /* tau_0 .. tau_{n-1} */ };

constexpr float k_dutyCycle = 0.5f;
constexpr float k_twoPi = 2.0f * 3.14159265358979323846f;

/* [1e-21 J] that the contribution leaves in the pixel during one exposure */
WPT_HD float energy(float pixelArea, float exposureTime, float radianceW)
{
    const float irradiance = radianceW * 1000.0f;
    const float power = irradiance * pixelArea;
    return power * k_dutyCycle * exposureTime;
}

/* the share that moves from tap b to tap a, for light that a ToF light modulated */
WPT_HD float modulation(float contrast, float fracModfreqC, float tau, float oplW)
{
    const float phaseShift = k_twoPi * oplW * fracModfreqC;
    return contrast * wptm::cosf_(tau + phaseShift);
}

/* acc = (a, b, total) */
WPT_HD void add(float energy, float t, float& a, float& b, float& total)
{
    const float halfEnergy = 0.5f * energy;
    const float energyA = halfEnergy * (1.0f + t);
    const float energyB = halfEnergy * (1.0f - t);
    a += energyA;
    b += energyB;
    total += energy;
}

} /* namespace wpttof */

#endif
