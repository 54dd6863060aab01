// Harness of tests/test_triangle_rotated.py: wurblpt_amd/csrc/wpt_triangle.h, triangleTest (corners in world order, components
// selected by the ray's axes) against triangleTestRotated (corners and origin in the order of the ray's kz, the swap as a sign
// flip), on uint32 views of accepted, a, invDet, U, V, W, with the ray's constants from rayAux / rayAuxRotated as the walk makes
// them and again as the light-pdf loop does (SHEAR_ONLY).  One line per set: cases, accepted, fall-back, differences.
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
    if (entersFallback(v0, v1, v2, org, h))
        t.fallback++;
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
    const long long N = argc > 1 ? atoll(argv[1]) : 100000000ll;
    unsigned long long bad = 0;

    /* random rays aimed at a point inside (or a little outside) a random triangle: about half of them hit */
    bad += report("random", run(N, 1, [](uint64_t& s, long long, Tally& t) {
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

    printf("total: %llu differences\n", bad);
    return bad == 0 ? 0 : 1;
}
