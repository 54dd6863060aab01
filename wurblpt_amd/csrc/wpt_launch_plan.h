/*
 * wpt_launch_plan.h -- which passes render a launch (host only; wpt_capi_render.hip).
 *
 * Where wpt_kernel_table.h says which kernel renders a launch, planLaunch says how it is launched: wavefront form or single
 * kernel, pixel pool or not, and one pass, two passes, one pass in the adaptive map's order, or pixels in slices.  A pure
 * function of its facts (no HIP call, nothing global, no header of the kernels), so that it is tested without a device
 * (wpt_launch_plan) and compiles on its own (tests/launch_plan_check.cpp).  DESIGN.md section 4, "Which passes render a launch",
 * has the rule as a table and what was measured for each line of it.  Where the memory a strategy needs cannot be had, the
 * launch falls back to ONE_PASS: that belongs to the execution, not to the plan.
 */
#ifndef WPT_LAUNCH_PLAN_H
#define WPT_LAUNCH_PLAN_H

#include <cmath>
#include <cstdint>

namespace wptk {

/* the kernels' WG and SLICE_SLOT_MASK (wpt_pathtrace.inc.h) and the sensors the rule names (wpt_kernel_table.h, Sensor), restated
 * for a file that includes none of their headers; wpt_capi.hip asserts that they agree */
constexpr uint32_t PLAN_WG = 256, PLAN_SLICE_SLOT_MAX = (1u << 28) - 1u;
constexpr uint32_t PLAN_FRAME = 0, PLAN_VIEWS = 2, PLAN_ADAPTIVE = 3, PLAN_SENSORS = 5;
/* units per pixel that slicesPlan aims for at most: the best of the sweep on the bench frame */
constexpr uint32_t SLICE_UNITS_TARGET = 15;

/* wpt_slices_plan (wurblpt_hip.h has the rule, DESIGN.md section 4 the measurements behind it) */
inline void slicesPlan(uint32_t blockSize, uint32_t lanesAtOnce, uint32_t samplesSqrt, uint32_t* units, uint32_t* rows)
{
    *units = 1;
    *rows = samplesSqrt > 0 ? samplesSqrt : 1u;
    if (lanesAtOnce == 0 || samplesSqrt < 8 || uint64_t(blockSize) < 2ull * lanesAtOnce || uint64_t(blockSize) > 64ull * lanesAtOnce)
        return;
    const double perLane = double(blockSize) / double(lanesAtOnce);
    uint32_t target = uint32_t(std::sqrt(0.5 * double(samplesSqrt) * double(samplesSqrt) / perLane));
    target = target > SLICE_UNITS_TARGET ? SLICE_UNITS_TARGET : target;
    if (target < 2)
        return;
    uint32_t r = (samplesSqrt + target - 1) / target;
    r = r < 2 ? 2 : r;
    *rows = r;
    *units = (samplesSqrt + r - 1) / r;
}

struct LaunchFacts {
    uint32_t sensor; /* wpt_kernel_table.h, Sensor */
    bool count, rgl, anim; /* the launch counts its work; the FEAT_RGL and FEAT_ANIM bits of its need */
    bool sceneInLds; /* KernelChoice::sceneInLds */
    uint32_t blockSize, samplesSqrt, cuCount;
    uint32_t variant, wfMode, slices; /* the words of wpt_set_launch_config, wpt_set_wavefront (mode) and wpt_set_slices */
};

enum Strategy : uint32_t { ONE_PASS, TWO_PASSES, ADAPTIVE_ORDER, SLICED };

struct LaunchPlan {
    bool wavefront;         /* trace and shade as two kernels; the rest of the plan is the single kernel's, which renders otherwise */
    bool wavefrontFallBack; /* the library's own choice: without its memory the single kernel renders; false: every error is reported */
    bool pooled;            /* the pixels are handed out from the pixel pool */
    Strategy strategy;
    uint32_t units, rows;   /* SLICED: units per pixel and rows of strata per unit; otherwise 1 and samplesSqrt */
    uint32_t passes;        /* wpt_last_render_passes of the single kernel */
};

inline LaunchPlan planLaunch(const LaunchFacts& f)
{
    const bool frame = f.sensor == PLAN_FRAME;
    const uint64_t lanes = uint64_t(f.cuCount) * 4u * PLAN_WG; /* lanes the device holds at once */
    const uint64_t block = f.blockSize, grid = (block + PLAN_WG - 1) / PLAN_WG;
    LaunchPlan p = { false, false, false, ONE_PASS, 1, f.samplesSqrt, 1 };
    /* the wavefront form exists for one frame without counters of a scene at rest; the library takes it for measured BRDFs
     * from 2^21 lanes on */
    p.wavefront = frame && !f.count && !f.anim && (f.wfMode == 1u || (f.wfMode == 0u && f.rgl && f.blockSize >= (1u << 21)));
    p.wavefrontFallBack = p.wavefront && f.wfMode != 1u;
    /* more workgroups than compute units: the pixels are handed out one by one; variant bit 0x10: never */
    p.pooled = !f.count && !(f.variant & 0x10u) && f.blockSize < 0x80000000u && grid > f.cuCount;
    const bool ordered = p.pooled && !(f.variant & 0x40u); /* variant bit 0x40: the plain order, one launch */
    if (f.sensor == PLAN_ADAPTIVE) {
        /* the costly pixels first: a pixel's work is known before the launch, whatever the scene kind */
        if (ordered)
            p.strategy = ADAPTIVE_ORDER;
    } else if (!f.sceneInLds) {
        /* a timed first row of strata, then the rest with the longest tiles first, where the end of the launch is a noticeable
         * part of it; not for a batch of views (carry, cost and order are indexed by the pixel of one frame) */
        if (ordered && f.sensor != PLAN_VIEWS && f.samplesSqrt >= 8 && block >= 2u * lanes && block <= 64u * lanes) {
            p.strategy = TWO_PASSES;
            p.passes = 2;
        }
    } else if (frame && !f.count && ordered && block > lanes && f.blockSize <= PLAN_SLICE_SLOT_MAX) {
        /* the scene in LDS: any order but the frame's own costs more than it gains, so the pixels go out in slices */
        uint32_t units = 1, rows = f.samplesSqrt;
        const uint32_t forced = f.slices & 0xffu;
        if (forced == 0) {
            slicesPlan(f.blockSize, uint32_t(lanes), f.samplesSqrt, &units, &rows);
        } else if (forced >= 2 && f.samplesSqrt > 0) {
            rows = (f.samplesSqrt + forced - 1) / forced;
            units = (f.samplesSqrt + rows - 1) / rows;
        }
        /* (the pool's counter runs past its last index by less than the lanes of the launch) */
        if (units >= 2 && uint64_t(units) * block + 2 * lanes < 0x100000000ull) {
            p.strategy = SLICED;
            p.units = units;
            p.rows = rows;
        }
    }
    return p;
}

} /* namespace wptk */

#endif
