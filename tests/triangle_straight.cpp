// Harness of tests/test_triangle_straight.py: wurblpt_amd/csrc/wpt_triangle.h, triangleTestRotated (early returns) against
// triangleTestRotatedStraight (the leaf pass of the kernels with the scene in LDS: one straight run, rejections combined at the
// end), on uint32 views of accepted, a, invDet, U, V, W, with the ray's constants from rayAuxRotated as the walk makes them.
//
// usage: triangle_straight CASES EXTRA N
// CASES holds the seven sets of `triangle_rotated --dump CASES N` (26 words per case, see tests/triangle_rotated.cpp); both forms
// run over every case, and the branching form's result must also be the one the file carries (the select form's).  Then one more
// set of N cases is made here and written to EXTRA in the same 26 words: ordinary hits and misses mixed with the cases in which
// the straight form computes what the branching form never reaches --
//   kind 0  an ordinary case of the "random" recipe
//   kind 1  det == 0: the three corners on the ray (U = V = W = 0, so 1 / det is infinite and a = inf * 0 is NaN, thrown away)
//   kind 2  a zero-area triangle, its third corner on the line of the first two: mixed signs or zeros, never accepted
//   kind 3  a NaN corner: every comparison is false and the case is ACCEPTED, as in the reference, with NaN words
//   kind 4  an infinite invDet: corners within 2^-62 of the origin, det denormal, accepted with a infinite or NaN
//   kind 5  amin at the case's own a or next to it      kind 6  amax there
// One line per set: cases, accepted, accepted by the straight form alone or the branching form alone, differing words; for the
// extra set also how many cases of each kind there are, how many of each are accepted, and in how many the straight form
// computed det == 0, an infinite invDet, a NaN.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_triangle.h"

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
static inline f3 rnd3(uint64_t& s, float r) { return mk3(sym(s, r), sym(s, r), sym(s, r)); }
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline bool isNan(uint32_t w) { return (w & 0x7fffffffu) > 0x7f800000u; }
static inline bool sameWord(uint32_t a, uint32_t b) { return a == b || (isNan(a) && isNan(b)); } /* which NaN is not covered */

constexpr int WORDS = 26;

struct Tally {
    unsigned long long cases = 0, accepted = 0, onlyStraight = 0, onlyBranching = 0, words = 0, notTheFiles = 0;
};

/* one case through both forms as the leaf pass calls them; out (may be null): the 26 words of the case */
static void one(const float in[17], const uint32_t* file, Tally& t, uint32_t* out)
{
    const f3 v0 = ld3(in), v1 = ld3(in + 3), v2 = ld3(in + 6), org = ld3(in + 9), dir = ld3(in + 12);
    const float amin = in[15], amax = in[16];
    const RayAux r = rayAuxRotated(dir);
    const int kz = auxKz(r);
    const uint32_t flip = (uint32_t)r.k & (uint32_t)RAY_FLIP;
    Candidate b, s;
    memset(&b, 0, sizeof b);
    memset(&s, 0, sizeof s);
    const bool hb = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), r.Sx, r.Sy, comp(r.inv, kz), flip, amin, amax, b);
    const bool hs = triangleTestRotatedStraight(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), r.Sx, r.Sy, comp(r.inv, kz), flip, amin, amax, s);
    t.cases++;
    if (hb)
        t.accepted++;
    if (hs && !hb)
        t.onlyStraight++;
    if (hb && !hs)
        t.onlyBranching++;
    const uint32_t wb[6] = { hb ? 1u : 0u, hb ? bits(b.a) : 0u, hb ? bits(b.invDet) : 0u, hb ? bits(b.U) : 0u, hb ? bits(b.V) : 0u, hb ? bits(b.W) : 0u };
    if (hb && hs) {
        const uint32_t ws[6] = { 1u, bits(s.a), bits(s.invDet), bits(s.U), bits(s.V), bits(s.W) };
        for (int i = 1; i < 6; i++)
            if (!sameWord(wb[i], ws[i]))
                t.words++;
    }
    if (file)
        for (int i = 0; i < 6; i++)
            if (!sameWord(wb[i], file[17 + i])) {
                t.notTheFiles++;
                break;
            }
    if (out) {
        memcpy(out, in, 17 * sizeof(float));
        memcpy(out + 17, wb, sizeof wb);
        const f3 A = sub(rotated(v0, kz), rotated(org, kz)), B = sub(rotated(v1, kz), rotated(org, kz)), C = sub(rotated(v2, kz), rotated(org, kz));
        const float Ax = A.x - r.Sx * A.z, Ay = A.y - r.Sy * A.z, Bx = B.x - r.Sx * B.z, By = B.y - r.Sy * B.z, Cx = C.x - r.Sx * C.z, Cy = C.y - r.Sy * C.z;
        const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax; /* |.| is the flipped form's too */
        out[23] = (__builtin_fabsf(U) < k_ldeps || __builtin_fabsf(V) < k_ldeps || __builtin_fabsf(W) < k_ldeps) ? 1u : 0u;
        out[24] = (uint32_t)rayAux(dir).k;
        out[25] = (uint32_t)r.k;
    }
}

static unsigned long long report(const char* name, const Tally& t)
{
    printf("%s: %llu cases, %llu accepted, %llu straight alone, %llu branching alone, %llu words differ, %llu not the file's\n", name, t.cases, t.accepted,
            t.onlyStraight, t.onlyBranching, t.words, t.notTheFiles);
    return t.onlyStraight + t.onlyBranching + t.words + t.notTheFiles;
}

/* the "random" recipe of tests/triangle_rotated.cpp: a ray aimed at a point inside or a little outside a random triangle */
static void ordinary(uint64_t& s, float in[17])
{
    const f3 v0 = rnd3(s, 10.0f), v1 = rnd3(s, 10.0f), v2 = rnd3(s, 10.0f), org = rnd3(s, 20.0f);
    const float u = 1.5f * unit(s) - 0.25f, v = 1.5f * unit(s) - 0.25f;
    const f3 target = add(v0, add(scl(u, sub(v1, v0)), scl(v, sub(v2, v0))));
    f3 dir = sub(target, org);
    const float len = __builtin_sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
    dir = mk3(dir.x / len, dir.y / len, dir.z / len);
    const float c[17] = { v0.x, v0.y, v0.z, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z, org.x, org.y, org.z, dir.x, dir.y, dir.z, 1e-4f, 3.402823466e+38f };
    memcpy(in, c, sizeof c);
}

int main(int argc, char** argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s CASES EXTRA cases-per-set\n", argv[0]);
        return 2;
    }
    const long long N = atoll(argv[3]);
    static const char* names[7] = { "random", "axis ties", "shared edges and vertices", "exact zeros", "double-precision fall-back", "denormal products",
        "interval ends" };
    FILE* f = fopen(argv[1], "rb");
    if (N <= 0 || !f) {
        perror(argv[1]);
        return 2;
    }
    unsigned long long bad = 0;
    std::vector<uint32_t> set((size_t)N * WORDS);
    for (int k = 0; k < 7; k++) {
        if (fread(set.data(), sizeof(uint32_t) * WORDS, (size_t)N, f) != (size_t)N) {
            fprintf(stderr, "%s: short file\n", argv[1]);
            return 2;
        }
        Tally t;
        for (long long i = 0; i < N; i++) {
            float in[17];
            memcpy(in, &set[(size_t)i * WORDS], sizeof in);
            one(in, &set[(size_t)i * WORDS], t, nullptr);
        }
        bad += report(names[k], t);
    }
    fclose(f);

    /* the extra set */
    Tally t;
    unsigned long long kinds[7] = { 0, 0, 0, 0, 0, 0, 0 }, zeroDet = 0, infiniteInvDet = 0, nanWords = 0, acceptedOfKind[7] = { 0, 0, 0, 0, 0, 0, 0 };
    uint64_t s = 8;
    for (long long i = 0; i < N; i++) {
        float in[17];
        const int kind = (int)(i % 7);
        ordinary(s, in);
        if (kind == 1) { /* the three corners on the ray, at small integer multiples of a power-of-two direction: U = V = W = 0 */
            const float d[3] = { (float)((int)(next(s) % 3) - 1), (float)((int)(next(s) % 3) - 1), (i & 8) ? 2.0f : -2.0f };
            const float o[3] = { (float)((int)(next(s) % 7) - 3), (float)((int)(next(s) % 7) - 3), (float)((int)(next(s) % 7) - 3) };
            const int p = (int)((i / 7) % 3); /* the largest component in every place */
            for (int c = 0; c < 3; c++) {
                in[9 + c] = o[(c + p) % 3];
                in[12 + c] = d[(c + p) % 3];
            }
            for (int v = 0; v < 3; v++)
                for (int c = 0; c < 3; c++)
                    in[3 * v + c] = in[9 + c] + (float)(v + 1) * in[12 + c];
            in[15] = -3.402823466e+38f;
        } else if (kind == 2) { /* a zero-area triangle: the third corner on the line of the first two */
            const float w = (i & 8) ? 0.5f : 2.0f;
            for (int c = 0; c < 3; c++) {
                in[c] = (float)((int)(next(s) % 9) - 4);
                in[3 + c] = in[c] + 2.0f * (float)((int)(next(s) % 5) - 2);
                in[6 + c] = in[c] + w * (in[3 + c] - in[c]);
            }
        } else if (kind == 3) {
            in[next(s) % 9] = __builtin_nanf("");
        } else if (kind == 4) {
            const float scale = ldexpf(1.0f, -62 - (int)(i % 3));
            const f3 o = rnd3(s, ldexpf(1.0f, -58));
            const f3 v0 = add(o, rnd3(s, scale)), v1 = add(o, rnd3(s, scale)), v2 = add(o, rnd3(s, scale));
            f3 d = sub(mk3((v0.x + v1.x + v2.x) / 3.0f, (v0.y + v1.y + v2.y) / 3.0f, (v0.z + v1.z + v2.z) / 3.0f), o);
            if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f)
                d = rnd3(s, 1.0f);
            const float c[17] = { v0.x, v0.y, v0.z, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z, o.x, o.y, o.z, d.x, d.y, d.z, -3.402823466e+38f, 3.402823466e+38f };
            memcpy(in, c, sizeof c);
        } else if (kind >= 5) { /* an accepted ordinary case again, an end of the interval at its a or next to it */
            Candidate c;
            while (!triangleTest(ld3(in), ld3(in + 3), ld3(in + 6), ld3(in + 9), rayAux(ld3(in + 12)), 1e-4f, 3.402823466e+38f, c))
                ordinary(s, in);
            const int e = (int)((i / 7) % 3);
            const float end = e == 0 ? nextafterf(c.a, -INFINITY) : (e == 1 ? c.a : nextafterf(c.a, INFINITY));
            in[kind == 5 ? 15 : 16] = end;
        }
        const unsigned long long before = t.accepted;
        one(in, nullptr, t, &set[(size_t)i * WORDS]);
        kinds[kind]++;
        acceptedOfKind[kind] += t.accepted - before;
        /* what the straight form computed where the branching form may have returned early: its c for this case */
        {
            const RayAux r = rayAuxRotated(ld3(in + 12));
            const int kz = auxKz(r);
            Candidate c;
            triangleTestRotatedStraight(rotated(ld3(in), kz), rotated(ld3(in + 3), kz), rotated(ld3(in + 6), kz), rotated(ld3(in + 9), kz), r.Sx, r.Sy,
                    comp(r.inv, kz), (uint32_t)r.k & (uint32_t)RAY_FLIP, in[15], in[16], c);
            if (c.U + c.V + c.W == 0.0f)
                zeroDet++;
            if (std::isinf(c.invDet))
                infiniteInvDet++;
            if (std::isnan(c.a) || std::isnan(c.U))
                nanWords++;
        }
    }
    bad += report("straight extras", t);
    printf("straight extras kinds: %llu %llu %llu %llu %llu %llu %llu, accepted %llu %llu %llu %llu %llu %llu %llu, det == 0 %llu, infinite invDet %llu, NaN %llu\n",
            kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], kinds[5], kinds[6], acceptedOfKind[0], acceptedOfKind[1], acceptedOfKind[2], acceptedOfKind[3],
            acceptedOfKind[4], acceptedOfKind[5], acceptedOfKind[6], zeroDet, infiniteInvDet, nanWords);
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(set.data(), sizeof(uint32_t) * WORDS, (size_t)N, g) != (size_t)N || fclose(g) != 0) {
        perror(argv[2]);
        return 2;
    }
    printf("total: %llu differences\n", bad);
    return bad == 0 ? 0 : 1;
}
