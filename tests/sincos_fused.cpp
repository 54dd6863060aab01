// Harness of tests/test_sincos_fused.py: wptm::sincosf_ (wurblpt_amd/csrc/wpt_math.h), the branch-free evaluation of a sine and a
// cosine of one angle, against wptm::sinf_ and wptm::cosf_ -- the functions tests/math_exact.cpp pins to the C library and the
// oracle evaluates -- on every one of the 2^32 float bit patterns.  Exhaustive: no tolerance, no sampling.
// With -DWPT_SINCOSF_POLY_BRANCH it checks the header's other form (shared reduction, polynomial chosen by branch).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <omp.h>

#include "../wurblpt_amd/csrc/wpt_math.h"

static inline float fromBits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t toBits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
    unsigned long long badSin = 0, badCos = 0;
#pragma omp parallel for schedule(static) reduction(+ : badSin, badCos)
    for (long long i = 0; i < (1ll << 32); i++) {
        volatile float x = fromBits((uint32_t)i); /* volatile: three separate evaluations of the argument as it is in memory */
        float s, c;
        wptm::sincosf_(x, &s, &c);
        if (toBits(s) != toBits(wptm::sinf_(x)))
            badSin++;
        if (toBits(c) != toBits(wptm::cosf_(x)))
            badCos++;
    }
    printf("sine of sincosf_ all 2^32 arguments: %llu differences\n", badSin);
    printf("cosine of sincosf_ all 2^32 arguments: %llu differences\n", badCos);
    printf("total: %llu differences\n", badSin + badCos);
    return badSin + badCos == 0 ? 0 : 1;
}
