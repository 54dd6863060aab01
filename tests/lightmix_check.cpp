/*
 * lightmix_check.cpp -- wurblpt_amd/csrc/wpt_lightmix.h on its own: compiled outside the library, without a header of HIP, with
 * -fsanitize=address,undefined, and run as a program (tests/test_light_groups_host.py).  Every buffer has exactly the size the
 * interface promises to stay within, so a read or write past it stops the program.
 *   - the host mix over random planes, strides and weights (negative, zero, minus zero, denormal, huge) against the same
 *     left-to-right expression written here with every product and sum forced through memory
 *   - the table check over random good tables and damaged ones: the verdict against one derived here another way, and the
 *     entry it names
 * Prints one line: "<mixes> mixes, <tables> tables (<bad> refused), <failures> failures".
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_lightmix.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t next()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(state >> 32);
}
static float unit() { return float(next() >> 8) * (1.0f / 16777216.0f); }

static float someWeight()
{
    switch (next() % 8) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return 1e-41f * float(next() % 100);   /* denormal */
    case 3: return -1e-40f;
    case 4: return -unit() * 4.0f;
    case 5: return 1e30f * unit();
    default: return unit() * 2.0f;
    }
}

static float somePlaneValue()
{
    switch (next() % 16) {
    case 0: return 0.0f;
    case 1: return 1e-42f * float(next() % 50);
    case 2: return 1e20f * unit();
    default: return unit() * 8.0f;
    }
}

static bool sameBits(float a, float b)
{
    uint32_t x, y;
    memcpy(&x, &a, 4);
    memcpy(&y, &b, 4);
    return x == y || (std::isnan(a) && std::isnan(b));
}

int main()
{
    unsigned long long mixes = 0, tables = 0, refused = 0, failures = 0;

    for (int round = 0; round < 3000; round++) {
        const uint32_t K = round < 3 ? (round == 0 ? 1u : round == 1 ? 3u : 17u) : 1u + next() % 40;
        const uint64_t pixels = 1 + next() % 37;
        const size_t stride = size_t(pixels) * 3 + (next() % 3 == 0 ? next() % 11 : 0);
        /* the last plane ends where its pixels end: nothing behind it belongs to the caller */
        std::vector<float> planes(size_t(K - 1) * stride + size_t(pixels) * 3), weights(size_t(K) * 3), out(size_t(pixels) * 3, -1.0f);
        for (float& v : planes)
            v = somePlaneValue();
        for (float& w : weights)
            w = someWeight();
        wptmix::mixHost(planes.data(), K, stride, pixels, weights.data(), out.data());
        for (size_t i = 0; i < out.size(); i++) {
            volatile float sum = 0.0f;
            for (uint32_t k = 0; k < K; k++) {
                volatile float term = weights[size_t(k) * 3 + i % 3] * planes[size_t(k) * stride + i];
                sum = sum + term;
            }
            if (!sameBits(out[i], sum)) {
                if (failures++ < 5)
                    printf("BROKEN mix: round %d value %zu: %a, expected %a\n", round, i, double(out[i]), double(sum));
            }
        }
        mixes++;
    }

    for (int round = 0; round < 200000; round++) {
        const uint32_t materials = next() % 40;
        uint32_t K = 1 + next() % 255;
        if (next() % 4 == 0)
            K = 1 + next() % 4;
        std::vector<uint8_t> table(materials);
        for (uint8_t& g : table)
            g = next() % 5 == 0 ? uint8_t(wptmix::GROUP_NONE) : uint8_t(next() % K);
        uint32_t env = next() % 3 == 0 ? uint32_t(wptmix::GROUP_NONE) : next() % K;
        /* damage: a count out of range, an entry or the environment's group out of range, or no table */
        const uint32_t damage = next() % 8;
        const uint8_t* given = materials ? table.data() : reinterpret_cast<const uint8_t*>(&state); /* no bytes are read of an empty table */
        if (damage == 1)
            K = next() % 2 ? 0u : 256u + next() % 1000;
        else if (damage == 2 && materials)
            table[next() % materials] = uint8_t(next());
        else if (damage == 3)
            env = next() % 2 ? next() : next() % 300;
        else if (damage == 4)
            given = nullptr;
        /* the verdict, derived in the order the check promises: no table, the count, the first bad entry, the environment */
        wptmix::TableError expect = wptmix::TABLE_OK;
        uint32_t expectAt = 0;
        if (!given) {
            expect = wptmix::TABLE_NULL;
        } else if (K < 1 || K > 255) {
            expect = wptmix::TABLE_GROUP_COUNT;
        } else {
            for (uint32_t m = materials; m-- > 0;)
                if (!(table[m] < K || table[m] == 0xff)) {
                    expect = wptmix::TABLE_ENTRY;
                    expectAt = m;
                }
            if (expect == wptmix::TABLE_OK && !(env < K || env == 0xff))
                expect = wptmix::TABLE_ENV_GROUP;
        }
        uint32_t at = 12345;
        const wptmix::TableError got = wptmix::checkTable(given, materials, K, env, &at);
        if (got != expect || at != expectAt || wptmix::checkTable(given, materials, K, env, nullptr) != expect) {
            if (failures++ < 5)
                printf("BROKEN table: round %d: verdict %d at %u, expected %d at %u\n", round, int(got), at, int(expect), expectAt);
        }
        tables++;
        refused += got != wptmix::TABLE_OK;
    }

    printf("%llu mixes, %llu tables (%llu refused), %llu failures\n", mixes, tables, refused, failures);
    return failures == 0 ? 0 : 1;
}
