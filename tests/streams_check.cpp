/*
 * streams_check.cpp -- wurblpt_amd/csrc/wpt_streams.h on its own: compiled outside the library, without a header of HIP, with
 * -Wall -Wextra -Werror and under the address and undefined-behaviour sanitizers (tests/test_streams_host.py).  Every buffer has
 * exactly the promised size, so a read or write outside it is reported.  Checks the mean, the moment and the merge against their
 * expressions written out here, and the split plan's promises over a sweep of frames, sample counts and devices.
 * Prints "<means> means <merges> merges <plans> plans <failures> failures".
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_streams.h"

static uint32_t bitsOf(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

/* bit for bit; a NaN matches a NaN (its sign and payload are the implementation's) */
static bool same(float a, float b)
{
    return (std::isnan(a) && std::isnan(b)) || bitsOf(a) == bitsOf(b);
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t next32()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(state >> 32);
}

static float someFloat()
{
    static const float specials[] = { INFINITY, -INFINITY, NAN, 1e-42f, -3e-45f, -0.0f, 0.0f, 3e38f, -3e38f };
    const uint32_t r = next32();
    if (r % 16 == 0)
        return specials[(r >> 8) % 9];
    return std::ldexp(float(int32_t(next32())) / 2147483648.0f, int(r >> 8) % 40 - 20);
}

int main()
{
    unsigned long long means = 0, merges = 0, plans = 0, failures = 0;
    const uint32_t counts[] = { 1, 2, 3, 16 };
    for (uint32_t K : counts) {
        for (size_t values : { size_t(1), size_t(3), size_t(63), size_t(192) }) {
            for (size_t gap : { size_t(0), size_t(5) }) {
                const size_t stride = values + gap;
                /* the last plane ends with its values: nothing behind it belongs to the planes */
                std::vector<float> planes((K - 1) * stride + values);
                for (float& v : planes)
                    v = someFloat();
                std::vector<float> mean(values), moment(values), meanOnly(values);
                wptstr::meanHost(planes.data(), K, stride, values, mean.data(), moment.data());
                wptstr::meanHost(planes.data(), K, stride, values, meanOnly.data(), nullptr);
                for (size_t i = 0; i < values; i++) {
                    volatile float sum = planes[i];
                    volatile float squares = planes[i] * planes[i];
                    for (uint32_t k = 1; k < K; k++) {
                        const float v = planes[k * stride + i];
                        volatile float square = v * v;
                        sum = sum + v;
                        squares = squares + square;
                    }
                    volatile float inv = 1.0f / float(K);
                    const float wantMean = sum * inv, wantMoment = squares * inv;
                    if (!same(mean[i], wantMean) || !same(moment[i], wantMoment) || !same(meanOnly[i], wantMean)) {
                        printf("BROKEN mean K %u value %zu\n", K, i);
                        failures++;
                    }
                    if (K == 1 && (!same(mean[i], planes[i]) || !same(moment[i], planes[i] * planes[i]))) {
                        printf("BROKEN one plane, value %zu\n", i);
                        failures++;
                    }
                    means++;
                }
            }
        }
    }
    for (int round = 0; round < 2000; round++) {
        const size_t values = 1 + next32() % 17;
        std::vector<float> a(values), b(values), out(values);
        for (size_t i = 0; i < values; i++) {
            a[i] = someFloat();
            b[i] = someFloat();
        }
        const uint32_t ca = round % 7 == 0 ? 0u : (round % 11 == 0 ? 0xffffffffu : next32() % 100);
        const uint32_t cb = ca == 0 ? 1 + next32() % 100 : (round % 11 == 0 ? 0xffffffffu : next32() % 100 + (ca == 0));
        wptstr::mergeHost(a.data(), ca, b.data(), cb, values, out.data());
        for (size_t i = 0; i < values; i++) {
            volatile float wa = float(ca) * a[i];
            volatile float wb = float(cb) * b[i];
            volatile float sum = wa + wb;
            const float want = sum / float(uint64_t(ca) + uint64_t(cb));
            if (!same(out[i], want)) {
                printf("BROKEN merge %u %u value %zu\n", ca, cb, i);
                failures++;
            }
            merges++;
        }
        /* in place */
        wptstr::mergeHost(a.data(), ca, b.data(), cb, values, a.data());
        for (size_t i = 0; i < values; i++)
            if (!same(a[i], out[i])) {
                printf("BROKEN merge in place\n");
                failures++;
            }
    }
    const uint64_t frames[] = { 1, 128, 37 * 23, 352 * 288, 320 * 200, 1024 * 1024, 0x7fffffffull, 0xffffffffffffffffull };
    const uint32_t devices[] = { 1, 1024, 65536, 262144, 0xffffffffu };
    for (uint64_t pixels : frames)
        for (uint32_t lanes : devices)
            for (uint32_t n = 1; n <= 260; n++) {
                uint32_t K = 0, ns = 0;
                bool ok = wptstr::splitPlan(pixels, n, lanes, &K, &ns);
                const uint32_t k = uint32_t(std::lround(std::sqrt(double(K))));
                ok = ok && K >= 1 && k * k == K && ns >= 1 && k * ns == n && uint64_t(K) * ns * ns == uint64_t(n) * n && (k == 1 || ns >= 2);
                /* no smaller admissible k reaches the aim, and a k that misses it is the largest admissible one */
                const long double aim = 4.0L * lanes;
                for (uint32_t j = 1; ok && j < k; j++)
                    if (n % j == 0 && (j == 1 || n / j >= 2) && (long double)j * j * pixels >= aim)
                        ok = false;
                if (ok && (long double)k * k * pixels < aim)
                    for (uint32_t j = k + 1; j <= n / 2; j++)
                        if (n % j == 0)
                            ok = false;
                if (!ok) {
                    printf("BROKEN plan pixels %llu n %u lanes %u: K %u ns %u\n", (unsigned long long)pixels, n, lanes, K, ns);
                    failures++;
                }
                plans++;
            }
    uint32_t K = 7, ns = 7;
    if (wptstr::splitPlan(0, 4, 4, &K, &ns) || wptstr::splitPlan(4, 0, 4, &K, &ns) || wptstr::splitPlan(4, 4, 0, &K, &ns) || K != 7 || ns != 7) {
        printf("BROKEN plan: a zero argument\n");
        failures++;
    }
    if (!wptstr::splitPlan(352 * 288, 16, 262144, &K, &ns) || K != 16 || ns != 4 || !wptstr::splitPlan(1024 * 1024, 32, 262144, &K, &ns) || K != 1
            || ns != 32 || !wptstr::splitPlan(352 * 288, 13, 262144, &K, &ns) || K != 1 || ns != 13) {
        printf("BROKEN plan: the three stated answers\n");
        failures++;
    }
    printf("%llu means %llu merges %llu plans %llu failures\n", means, merges, plans, failures);
    return failures ? 1 : 0;
}
