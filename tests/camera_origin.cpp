// Harness of tests/test_camera_origin.py: wurblpt_amd/csrc/wpt_camera_origin.h, cameraOriginAtRest -- the origin of a camera's
// rays as the large form of the kernels with the scene in LDS evaluates it once per launch -- against the expression that
// blockNewFrom (wpt_blocks.h) evaluates per sample for a camera at rest without a lens, written out here as it stands there, on
// uint32 views of the three words.  A third evaluation takes the zero vector from volatile memory, so that the compiler folds
// nothing of it: what it may have folded of the literal zeros in the other two must be what the arithmetic gives.
//
// usage: camera_origin N [SEED]
// N random poses (translation within +-100, a unit quaternion, scaling within +-10 per axis), then the adversarial set: every
// combination of
//   translation components  0, -0, 1.5, -3
//   scaling components      1, -2, 0, -0, a denormal, +inf, -inf, NaN
//   quaternions             identity, a unit rotation, the same times 3, times 2^-70, times 2^70, and all zeros (non-unit ones
//                           are not normalised by anybody: gvm.hpp's rotation is applied as it is)
// A word counts as equal if the bits are equal or both are NaN (which NaN is not covered, as in wpt_triangle.h's tests).
// One line per set: cases, differing words of the function, differing words of the unfolded evaluation, and in how many cases
// the origin is NOT the translation bit for bit (so that "the origin is the translation" would have been a wrong short cut).
// Exit status 1 if a word differs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../wurblpt_amd/csrc/wpt_camera_origin.h"

using namespace wptd;

static inline uint64_t next(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline float unit(uint64_t& s) { return (float)(next(s) >> 40) * 5.9604644775390625e-08f; } /* [0, 1) */
static inline float sym(uint64_t& s, float r) { return (2.0f * unit(s) - 1.0f) * r; }
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline bool isNan(uint32_t w) { return (w & 0x7fffffffu) > 0x7f800000u; }
static inline bool sameWord(float a, float b) { return bits(a) == bits(b) || (isNan(bits(a)) && isNan(bits(b))); }

struct Tally {
    unsigned long long cases = 0, words = 0, unfolded = 0, notTheTranslation = 0;
};

static volatile float g_zero[3] = { 0.0f, 0.0f, 0.0f };

static void one(const wpt_camera& cam, Tally& t)
{
    const f3 got = cameraOriginAtRest(cam);
    /* blockNewFrom, the branch of a camera at rest, with O as the lens-less path leaves it */
    const f3 O = mk3(0.0f, 0.0f, 0.0f);
    const float rotation[4] = { cam.rotation[0], cam.rotation[1], cam.rotation[2], cam.rotation[3] };
    const f3 translation = mk3(cam.translation[0], cam.translation[1], cam.translation[2]);
    const f3 scaling = mk3(cam.scaling[0], cam.scaling[1], cam.scaling[2]);
    const f3 want = add(translation, quatRotate(rotation, mul(O, scaling)));
    const f3 Ov = mk3(g_zero[0], g_zero[1], g_zero[2]);
    const f3 plain = add(translation, quatRotate(rotation, mul(Ov, scaling)));
    t.cases++;
    t.words += !sameWord(got.x, want.x) + !sameWord(got.y, want.y) + !sameWord(got.z, want.z);
    t.unfolded += !sameWord(got.x, plain.x) + !sameWord(got.y, plain.y) + !sameWord(got.z, plain.z);
    if (bits(got.x) != bits(translation.x) || bits(got.y) != bits(translation.y) || bits(got.z) != bits(translation.z))
        t.notTheTranslation++;
}

static void report(const char* name, const Tally& t)
{
    printf("%s: %llu cases, %llu words differ, %llu from the unfolded evaluation, %llu not the translation\n", name, t.cases, t.words, t.unfolded,
            t.notTheTranslation);
}

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    uint64_t s = argc > 2 ? strtoull(argv[2], nullptr, 0) : 20240607ull;
    Tally random, adversarial;
    wpt_camera cam;
    memset(&cam, 0, sizeof cam);
    for (long i = 0; i < n; i++) {
        float q[4], len = 0.0f;
        do {
            len = 0.0f;
            for (int k = 0; k < 4; k++) {
                q[k] = sym(s, 1.0f);
                len += q[k] * q[k];
            }
        } while (len < 1e-3f || len > 1.0f);
        len = std::sqrt(len);
        for (int k = 0; k < 4; k++)
            cam.rotation[k] = q[k] / len;
        for (int k = 0; k < 3; k++) {
            cam.translation[k] = sym(s, 100.0f);
            cam.scaling[k] = sym(s, 10.0f);
        }
        one(cam, random);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float T[4] = { 0.0f, -0.0f, 1.5f, -3.0f };
    const float S[8] = { 1.0f, -2.0f, 0.0f, -0.0f, 1e-41f, inf, -inf, nan };
    const float r[4] = { 0.18257419f, 0.36514837f, 0.54772256f, 0.73029674f }; /* (1, 2, 3, 4) / sqrt(30) */
    const float factors[4] = { 1.0f, 3.0f, 0x1p-70f, 0x1p70f };
    float Q[6][4] = { { 0.0f, 0.0f, 0.0f, 1.0f }, {}, {}, {}, {}, { 0.0f, 0.0f, 0.0f, 0.0f } };
    for (int f = 0; f < 4; f++)
        for (int k = 0; k < 4; k++)
            Q[1 + f][k] = r[k] * factors[f];
    for (int q = 0; q < 6; q++)
        for (int t = 0; t < 64; t++)
            for (int c = 0; c < 512; c++) {
                for (int k = 0; k < 4; k++)
                    cam.rotation[k] = Q[q][k];
                for (int k = 0; k < 3; k++) {
                    cam.translation[k] = T[(t >> (2 * k)) & 3];
                    cam.scaling[k] = S[(c >> (3 * k)) & 7];
                }
                one(cam, adversarial);
            }
    report("random", random);
    report("adversarial", adversarial);
    const unsigned long long bad = random.words + random.unfolded + adversarial.words + adversarial.unfolded;
    printf("total: %llu differences\n", bad);
    return bad ? 1 : 0;
}
