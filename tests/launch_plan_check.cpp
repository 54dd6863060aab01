/* launch_plan_check.cpp -- planLaunch (wurblpt_amd/csrc/wpt_launch_plan.h) on its own, built with -fsanitize=address,undefined by
 * tests/test_launch_plan.py and run as a program.  Sweeps the plan over the cross product of the values on both sides of each
 * threshold of its rule ("Which passes render a launch") and checks what must hold of every plan:
 *   one strategy out of four; SLICED implies units >= 2, rows * units >= samplesSqrt, the scene in LDS and the frame sensor;
 *   TWO_PASSES implies the scene in HBM and 2 passes, every other strategy 1; ADAPTIVE_ORDER implies the adaptive sensor;
 *   a launch without a pool, a counting launch among them, is ONE_PASS; the wavefront form is for one frame without counters
 *   of a scene at rest, and falls back only where the library chose it.
 * Prints a summary; exit status 1 if a plan breaks a rule. */
#include <cstdio>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_launch_plan.h"

using namespace wptk;

static long failures = 0;

static void check(bool ok, const char* rule, const LaunchFacts& f, const LaunchPlan& p)
{
    if (ok)
        return;
    if (failures++ < 20)
        printf("BROKEN %s: sensor %u count %d rgl %d anim %d lds %d block %u s %u cu %u variant %#x wf %u slices %#x -> wf %d/%d pooled %d strategy %u "
               "units %u rows %u passes %u\n", rule, f.sensor, f.count, f.rgl, f.anim, f.sceneInLds, f.blockSize, f.samplesSqrt, f.cuCount,
                f.variant, f.wfMode, f.slices, p.wavefront, p.wavefrontFallBack, p.pooled, unsigned(p.strategy), p.units, p.rows, p.passes);
}

int main()
{
    long plans = 0, byStrategy[4] = { 0, 0, 0, 0 }, wavefront = 0;
    for (uint32_t cu : { 8u, 256u, 131073u }) {
        const uint64_t lanes = uint64_t(cu) * 1024;
        std::vector<uint32_t> blocks = { 1u, 64u * 64u, cu * 256u, cu * 256u + 1u, (1u << 21) - 1u, 1u << 21, (1u << 28) - 1u, 1u << 28, 0x7fffffffu,
            0x80000000u, 0xffffffffu };
        for (uint64_t b : { lanes, lanes + 1, 2 * lanes - 1, 2 * lanes, 64 * lanes, 64 * lanes + 1 })
            if (b <= 0xffffffffull)
                blocks.push_back(uint32_t(b));
        for (uint32_t block : blocks)
            for (uint32_t s : { 1u, 7u, 8u, 32u, 45u, 65535u })
                for (uint32_t sensor = 0; sensor < PLAN_SENSORS; sensor++)
                    for (uint32_t bits = 0; bits < 16; bits++) /* count, rgl, anim, sceneInLds */
                        for (uint32_t variant : { 0u, 0x10u, 0x40u, 0x50u, 0xafu })
                            for (uint32_t wfMode = 0; wfMode < 3; wfMode++)
                                for (uint32_t slices : { 0u, 1u, 2u, 15u, 0x102u }) {
                                    const LaunchFacts f = { sensor, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, block, s, cu,
                                        variant, wfMode, slices };
                                    const LaunchPlan p = planLaunch(f);
                                    plans++;
                                    check(p.strategy <= SLICED, "one strategy out of four", f, p);
                                    if (p.strategy > SLICED)
                                        continue;
                                    byStrategy[p.strategy]++;
                                    wavefront += p.wavefront;
                                    const bool sliced = p.strategy == SLICED, two = p.strategy == TWO_PASSES;
                                    check(!sliced || (p.units >= 2 && p.units <= 15 && uint64_t(p.rows) * p.units >= s && uint64_t(p.rows) * (p.units - 1) < s),
                                            "a sliced launch's units cover the rows of strata", f, p);
                                    check(sliced || (p.units == 1 && p.rows == s), "units and rows of a launch that is not sliced", f, p);
                                    check(!sliced || (f.sceneInLds && f.sensor == PLAN_FRAME && uint64_t(p.units) * block + 2 * lanes < (1ull << 32)),
                                            "slices are for the frame sensor with the scene in LDS, and the pool's counter does not wrap", f, p);
                                    check(!two || (!f.sceneInLds && f.sensor != PLAN_VIEWS && f.sensor != PLAN_ADAPTIVE), "two passes need the scene in HBM", f, p);
                                    check(p.passes == (two ? 2u : 1u), "passes", f, p);
                                    check((p.strategy == ADAPTIVE_ORDER) == (f.sensor == PLAN_ADAPTIVE && p.pooled && !(variant & 0x40u)), "the adaptive order", f, p);
                                    check(p.pooled || p.strategy == ONE_PASS, "without a pool one pass", f, p);
                                    check(!(f.count || (variant & 0x10u) || block >= 0x80000000u) || !p.pooled, "no pool", f, p);
                                    check(!(variant & 0x40u) || p.strategy == ONE_PASS, "variant bit 0x40 is the plain order", f, p);
                                    check(!p.wavefront || (f.sensor == PLAN_FRAME && !f.count && !f.anim && wfMode != 2), "where the wavefront form exists", f, p);
                                    check(p.wavefrontFallBack == (p.wavefront && wfMode == 0), "only the library's own choice falls back", f, p);
                                }
    }
    printf("%ld plans: %ld one pass, %ld two passes, %ld adaptive order, %ld sliced; %ld in the wavefront form; %ld failures\n", plans, byStrategy[0],
            byStrategy[1], byStrategy[2], byStrategy[3], wavefront, failures);
    return failures || !byStrategy[1] || !byStrategy[2] || !byStrategy[3] || !wavefront ? 1 : 0;
}
