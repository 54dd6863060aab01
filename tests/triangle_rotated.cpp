// Harness of tests/test_triangle_rotated.py: wurblpt_amd/csrc/wpt_triangle.h, triangleTest (corners in world order, components
// selected by the ray's axes) against triangleTestRotated (corners and origin in the order of the ray's kz, the swap as a sign
// flip), on uint32 views of accepted, a, invDet, U, V, W, with the ray's constants from rayAux / rayAuxRotated as the walk makes
// them and again as the light-pdf loop does (SHEAR_ONLY).  One line per set: cases, accepted, fall-back, differences.
//
// Second mode, `triangle_rotated --dump FILE N`: the first N cases of every set, made by one thread from the set's seed, written
// to FILE for the tests that give them to the device (tests/test_gpu_triangle.py) or evaluate them exactly
// (tests/test_triangle_exact.py).  Per case 26 words of 32 bits: the 17 floats of the case (v0, v1, v2, origin, direction, amin,
// amax), the select form's host result (accepted, then the bits of a, invDet, U, V, W, zero when rejected), 1 where the case enters
// the double-precision fall-back, RayAux::k of rayAux and of rayAuxRotated.  The sets follow one another in the order of main().
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <omp.h>

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
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Tally {
    unsigned long long cases = 0, accepted = 0, fallback = 0, swapped = 0, bad = 0;
    unsigned long long perKz[3] = { 0, 0, 0 };
};

/* does triangleTest take its double-precision fall-back for this case?  (its first lines, single precision) */
static inline bool entersFallback(f3 v0, f3 v1, f3 v2, f3 org, const RayAux& h)
{
    const f3 A = sub(v0, org), B = sub(v1, org), C = sub(v2, org);
    const int kx = auxKx(h), ky = auxKy(h), kz = auxKz(h);
    const float Ax = comp(A, kx) - h.Sx * comp(A, kz), Ay = comp(A, ky) - h.Sy * comp(A, kz);
    const float Bx = comp(B, kx) - h.Sx * comp(B, kz), By = comp(B, ky) - h.Sy * comp(B, kz);
    const float Cx = comp(C, kx) - h.Sx * comp(C, kz), Cy = comp(C, ky) - h.Sy * comp(C, kz);
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    return __builtin_fabsf(U) < k_ldeps || __builtin_fabsf(V) < k_ldeps || __builtin_fabsf(W) < k_ldeps;
}

/* --dump: where one() writes the cases it sees, and how many the set still owes */
struct Dump {
    FILE* file = nullptr;
    long long left = 0;
};
static Dump g_dump;

static inline void dumpCase(f3 v0, f3 v1, f3 v2, f3 org, f3 dir, float amin, float amax, bool accepted, const Candidate& c, bool fallback, int k, int kRotated)
{
    if (!g_dump.file || g_dump.left <= 0)
        return;
    const float in[17] = { v0.x, v0.y, v0.z, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z, org.x, org.y, org.z, dir.x, dir.y, dir.z, amin, amax };
    uint32_t w[26];
    memcpy(w, in, sizeof in);
    w[17] = accepted ? 1u : 0u;
    w[18] = accepted ? bits(c.a) : 0u;
    w[19] = accepted ? bits(c.invDet) : 0u;
    w[20] = accepted ? bits(c.U) : 0u;
    w[21] = accepted ? bits(c.V) : 0u;
    w[22] = accepted ? bits(c.W) : 0u;
    w[23] = fallback ? 1u : 0u;
    w[24] = (uint32_t)k;
    w[25] = (uint32_t)kRotated;
    if (fwrite(w, sizeof w, 1, g_dump.file) != 1) {
        perror("--dump");
        exit(2);
    }
    g_dump.left--;
}

/* one case through both forms */
static inline void one(f3 v0, f3 v1, f3 v2, f3 org, f3 dir, float amin, float amax, Tally& t)
{
    const RayAux h = rayAux(dir);
    const RayAux r = rayAuxRotated(dir);
    const int kz = auxKz(r);
    Candidate a, b;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    const bool ha = triangleTest(v0, v1, v2, org, h, amin, amax, a);
    const bool hb = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), r.Sx, r.Sy, comp(r.inv, kz),
            (uint32_t)r.k & (uint32_t)RAY_FLIP, amin, amax, b);
    t.cases++;
    t.perKz[kz]++;
    if ((uint32_t)r.k & (uint32_t)RAY_FLIP)
        t.swapped++;
    if (ha)
        t.accepted++;
    const bool fallback = entersFallback(v0, v1, v2, org, h);
    if (fallback)
        t.fallback++;
    dumpCase(v0, v1, v2, org, dir, amin, amax, ha, a, fallback, h.k, r.k);
    bool same = ha == hb && auxKz(h) == kz;
    if (ha && hb)
        same = same && bits(a.a) == bits(b.a) && bits(a.invDet) == bits(b.invDet) && bits(a.U) == bits(b.U) && bits(a.V) == bits(b.V) && bits(a.W) == bits(b.W);
    /* the light-pdf loop's forms (SHEAR_ONLY: one division, its result in all of inv, inv.x taken as Sz), as hotSpotPdfValue and
     * hotSpotPdfValueRotated call the tests */
    const RayAux hs = rayAux<true>(dir);
    const RayAux rs = rayAuxRotated<true>(dir);
    Candidate as, bs;
    memset(&as, 0, sizeof as);
    memset(&bs, 0, sizeof bs);
    const bool has = triangleTest(v0, v1, v2, org, hs, amin, amax, as);
    const bool hbs = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), rs.Sx, rs.Sy, rs.inv.x,
            (uint32_t)rs.k & (uint32_t)RAY_FLIP, amin, amax, bs);
    same = same && has == hbs && has == ha && auxKz(rs) == kz && ((uint32_t)rs.k & (uint32_t)RAY_FLIP) == ((uint32_t)r.k & (uint32_t)RAY_FLIP);
    if (has && hbs)
        same = same && bits(as.a) == bits(bs.a) && bits(as.invDet) == bits(bs.invDet) && bits(as.U) == bits(bs.U) && bits(as.V) == bits(bs.V) && bits(as.W) == bits(bs.W)
                && bits(as.a) == bits(a.a) && bits(as.U) == bits(a.U);
    if (!same)
        t.bad++;
}

static void add(Tally& to, const Tally& t)
{
    to.cases += t.cases; to.accepted += t.accepted; to.fallback += t.fallback; to.swapped += t.swapped; to.bad += t.bad;
    for (int k = 0; k < 3; k++)
        to.perKz[k] += t.perKz[k];
}
static unsigned long long report(const char* name, const Tally& t)
{
    printf("%s: %llu cases, %llu accepted, %llu fall-back, %llu swapped, kz %llu %llu %llu, %llu differences\n", name, t.cases, t.accepted, t.fallback, t.swapped,
            t.perKz[0], t.perKz[1], t.perKz[2], t.bad);
    fflush(stdout);
    return t.bad;
}

template<class Case> static Tally run(long long count, uint64_t seed, Case make)
{
    Tally total;
    if (g_dump.file) { /* --dump: `count` cases, whatever the number of threads */
        uint64_t s = seed;
        g_dump.left = count;
        for (long long i = 0; g_dump.left > 0; i++)
            make(s, i, total);
        return total;
    }
#pragma omp parallel
    {
        Tally t;
        uint64_t s = seed + 7919ull * (uint64_t)omp_get_thread_num();
#pragma omp for schedule(static)
        for (long long i = 0; i < count; i++)
            make(s, i, t);
#pragma omp critical
        add(total, t);
    }
    return total;
}

static inline f3 rnd3(uint64_t& s, float r) { return mk3(sym(s, r), sym(s, r), sym(s, r)); }

int main(int argc, char** argv)
{
    const bool dump = argc == 4 && strcmp(argv[1], "--dump") == 0;
    if (argc > 1 && argv[1][0] == '-' && !dump) {
        fprintf(stderr, "usage: %s [cases of the random set] | --dump FILE cases-per-set\n", argv[0]);
        return 2;
    }
    /* --dump runs every set for 20 N cases, which each of them divides by 20 again */
    const long long N = dump ? 20 * atoll(argv[3]) : (argc > 1 ? atoll(argv[1]) : 100000000ll);
    if (dump && (N <= 0 || !(g_dump.file = fopen(argv[2], "wb")))) {
        perror(argv[2]);
        return 2;
    }
    unsigned long long bad = 0;

    /* random rays aimed at a point inside (or a little outside) a random triangle: about half of them hit */
    bad += report("random", run(dump ? N / 20 : N, 1, [](uint64_t& s, long long, Tally& t) {
        const f3 v0 = rnd3(s, 10.0f), v1 = rnd3(s, 10.0f), v2 = rnd3(s, 10.0f), org = rnd3(s, 20.0f);
        const float u = 1.5f * unit(s) - 0.25f, v = 1.5f * unit(s) - 0.25f;
        const f3 target = add(v0, add(scl(u, sub(v1, v0)), scl(v, sub(v2, v0))));
        f3 dir = sub(target, org);
        const float len = __builtin_sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
        dir = mk3(dir.x / len, dir.y / len, dir.z / len);
        one(v0, v1, v2, org, dir, 1e-4f, 3.402823466e+38f, t);
    }));

    /* the kz ties of rayAux: direction components that are zero, negative zero or equal in magnitude, every sign */
    bad += report("axis ties", run(N / 20, 2, [](uint64_t& s, long long i, Tally& t) {
        const float m = (i & 64) ? 1.0f : 0.25f + unit(s);
        const float pick[6] = { 0.0f, -0.0f, m, -m, 0.5f * m, -0.5f * m };
        f3 dir = mk3(pick[i % 6], pick[(i / 6) % 6], pick[(i / 36) % 6]);
        if (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f)
            dir.z = (i & 1) ? m : -m;
        const f3 org = rnd3(s, 4.0f);
        /* a triangle around a point on the ray, so that many are hit */
        const f3 c = add(org, scl(1.0f + 3.0f * unit(s), dir));
        one(add(c, rnd3(s, 2.0f)), add(c, rnd3(s, 2.0f)), add(c, rnd3(s, 2.0f)), org, dir, 0.0f, 3.402823466e+38f, t);
    }));

    /* rays through a vertex or a point of an edge of two triangles that share it */
    bad += report("shared edges and vertices", run(N / 20, 3, [](uint64_t& s, long long i, Tally& t) {
        const f3 v0 = rnd3(s, 8.0f), v1 = rnd3(s, 8.0f), v2 = rnd3(s, 8.0f), v3 = rnd3(s, 8.0f), org = rnd3(s, 16.0f);
        const float w = (i & 1) ? 0.0f : ((i & 2) ? 1.0f : unit(s));
        const f3 target = add(v0, scl(w, sub(v1, v0))); /* on the edge v0 v1, or one of its ends */
        const f3 dir = sub(target, org);                /* not normalized: the target is on the ray as exactly as floats allow */
        one(v0, v1, v2, org, dir, 0.0f, 3.402823466e+38f, t);
        one(v1, v0, v3, org, dir, 0.0f, 3.402823466e+38f, t);
    }));

    /* small integers: U, V, W are exact, often exactly zero (the ray runs through corners and edges), with either sign of zero
     * in the products; directions along an axis or a diagonal, both signs (the swap) */
    bad += report("exact zeros", run(N / 20, 4, [](uint64_t& s, long long i, Tally& t) {
        auto in = [&](int r) { return (float)((int)(next(s) % (uint64_t)(2 * r + 1)) - r); };
        const f3 v0 = mk3(in(3), in(3), in(3)), v1 = mk3(in(3), in(3), in(3)), v2 = mk3(in(3), in(3), in(3));
        const f3 org = mk3(in(3), in(3), in(3));
        f3 dir = mk3(in(1), in(1), in(1));
        if (i & 4)
            dir = mk3(dir.x * 2.0f, dir.y, dir.z * 4.0f);
        if (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f)
            dir.x = (i & 1) ? 1.0f : -1.0f;
        if (i & 8) /* zeros of either sign in the direction */
            dir = mk3(dir.x == 0.0f ? -0.0f : dir.x, dir.y == 0.0f ? -0.0f : dir.y, dir.z == 0.0f ? -0.0f : dir.z);
        one(v0, v1, v2, org, dir, -3.402823466e+38f, 3.402823466e+38f, t);
    }));

    /* tiny triangles close to the origin of the ray: |U|, |V| or |W| below 2^-63, the double-precision fall-back */
    bad += report("double-precision fall-back", run(N / 20, 5, [](uint64_t& s, long long i, Tally& t) {
        const float scale = ldexpf(1.0f, -28 - (int)(i % 12));
        const f3 org = rnd3(s, 1.0f);
        const f3 v0 = add(org, rnd3(s, scale)), v1 = add(org, rnd3(s, scale)), v2 = add(org, rnd3(s, scale));
        const f3 c = mk3((v0.x + v1.x + v2.x) / 3.0f, (v0.y + v1.y + v2.y) / 3.0f, (v0.z + v1.z + v2.z) / 3.0f);
        f3 dir = sub(c, org);
        if (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f)
            dir = rnd3(s, 1.0f);
        one(v0, v1, v2, org, dir, -3.402823466e+38f, 3.402823466e+38f, t);
    }));

    /* products of two numbers near 2^-62: the differences U, V, W are denormal or zero in single precision, det often so small
     * that invDet is infinite (and a = invDet * T infinite or NaN); every case enters the fall-back */
    bad += report("denormal products", run(N / 20, 6, [](uint64_t& s, long long i, Tally& t) {
        const float scale = ldexpf(1.0f, -60 - (int)(i % 4));
        const f3 org = rnd3(s, ldexpf(1.0f, -58));
        const f3 v0 = add(org, rnd3(s, scale)), v1 = add(org, rnd3(s, scale)), v2 = add(org, rnd3(s, scale));
        const f3 c = mk3((v0.x + v1.x + v2.x) / 3.0f, (v0.y + v1.y + v2.y) / 3.0f, (v0.z + v1.z + v2.z) / 3.0f);
        f3 dir = sub(c, org);
        if (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f)
            dir = rnd3(s, 1.0f);
        one(v0, v1, v2, org, dir, -3.402823466e+38f, 3.402823466e+38f, t);
    }));

    /* accepted cases of the random set again, with amin or amax at the case's own a or at one of the two floats next to it:
     * Ts < amin * ds and Ts > amax * ds are decided at or next to equality */
    bad += report("interval ends", run(N / 20, 7, [](uint64_t& s, long long i, Tally& t) {
        for (;;) {
            const f3 v0 = rnd3(s, 10.0f), v1 = rnd3(s, 10.0f), v2 = rnd3(s, 10.0f), org = rnd3(s, 20.0f);
            const float u = 1.5f * unit(s) - 0.25f, v = 1.5f * unit(s) - 0.25f;
            const f3 target = add(v0, add(scl(u, sub(v1, v0)), scl(v, sub(v2, v0))));
            f3 dir = sub(target, org);
            const float len = __builtin_sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
            dir = mk3(dir.x / len, dir.y / len, dir.z / len);
            Candidate c;
            if (!triangleTest(v0, v1, v2, org, rayAux(dir), 1e-4f, 3.402823466e+38f, c))
                continue;
            const float end = (i % 3) == 0 ? nextafterf(c.a, -INFINITY) : ((i % 3) == 1 ? c.a : nextafterf(c.a, INFINITY));
            if ((i / 3) & 1)
                one(v0, v1, v2, org, dir, 1e-4f, end, t);
            else
                one(v0, v1, v2, org, dir, end, 3.402823466e+38f, t);
            return;
        }
    }));

    if (dump && fclose(g_dump.file) != 0) {
        perror(argv[2]);
        return 2;
    }
    printf("total: %llu differences\n", bad);
    return bad == 0 ? 0 : 1;
}
