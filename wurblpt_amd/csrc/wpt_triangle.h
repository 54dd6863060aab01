/*
 * wpt_triangle.h -- the vector basics and the watertight triangle test of the gfx950 path tracer, in a header of their own so
 * that a host compiler can include them (tests/triangle_rotated.cpp compares the two forms of the test bit for bit on the CPU).
 * Like wpt_math.h it compiles as device code under hipcc and as plain C++ elsewhere; wpt_device.h includes it.
 */
#ifndef WPT_TRIANGLE_H
#define WPT_TRIANGLE_H

#include <stdint.h>

#include "wpt_math.h"

#if defined(__HIPCC__)
#define WPT_D __device__ __forceinline__
#else
#define WPT_D inline
#endif

namespace wptd {

constexpr float k_pi = 3.1415926535897932384626433832795029L;
constexpr float k_pi_2 = 1.5707963267948966192313216916397514L;
constexpr float k_pi_4 = 0.7853981633974483096156608458198757L;
constexpr float k_inv_pi = 0.3183098861837906715377675267450287L;
constexpr float k_maxval = 3.402823466e+38f;
constexpr float k_epsilon = 1.1920928955078125e-07f;
constexpr float k_ldeps = 1.084202172485504434e-19f; /* float(epsilon of long double), hitable_triangle.hpp:240 */

struct f2 { float x, y; };
struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

/* comparison-based min / max, NaN behaviour of gvm.hpp:88,93 */
WPT_D float fminr(float x, float y) { return x < y ? x : y; }
WPT_D float fmaxr(float x, float y) { return x > y ? x : y; }
WPT_D float clampr(float x, float lo, float hi) { return fminr(hi, fmaxr(lo, x)); }
WPT_D float mixr(float x, float y, float a) { return x + a * (y - x); }

WPT_D f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
WPT_D f4 mk4(float x, float y, float z, float w) { f4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
WPT_D f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
WPT_D f4 ld4(const float* p) { return mk4(p[0], p[1], p[2], p[3]); }
WPT_D f3 add(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
WPT_D f3 sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
WPT_D f3 mul(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
WPT_D f3 neg(f3 a) { return mk3(-a.x, -a.y, -a.z); }
WPT_D f3 scl(float s, f3 a) { return mk3(s * a.x, s * a.y, s * a.z); }    /* s * v */
WPT_D f3 sclr(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }   /* v * s */
WPT_D f3 divs(f3 a, float s) { return mk3(a.x / s, a.y / s, a.z / s); }
WPT_D f4 add(f4 a, f4 b) { return mk4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
WPT_D f4 sub(f4 a, f4 b) { return mk4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
WPT_D f4 mul(f4 a, f4 b) { return mk4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
WPT_D f4 scl(float s, f4 a) { return mk4(s * a.x, s * a.y, s * a.z, s * a.w); }
WPT_D f4 sclr(f4 a, float s) { return mk4(a.x * s, a.y * s, a.z * s, a.w * s); }
WPT_D f4 divs(f4 a, float s) { return mk4(a.x / s, a.y / s, a.z / s, a.w / s); }
WPT_D f3 cross(f3 v, f3 w) { return mk3(v.y * w.z - v.z * w.y, v.z * w.x - v.x * w.z, v.x * w.y - v.y * w.x); }
/* quaternion (x, y, z, w) rotates v, gvm.hpp:1713-1720 */
WPT_D f3 quatRotate(const float* q, f3 v)
{
    f3 s = mk3(q[0], q[1], q[2]);
    f3 t = scl(2.0f, cross(s, v));
    return add(add(v, scl(q[3], t)), cross(s, t));
}
WPT_D float comp(f3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
WPT_D float comp(f4 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : (i == 2 ? a.z : a.w)); }

/* RayIntersectionHelper (hitable.hpp:66-113) */
/* Kept per ray in registers while it traverses, so it is small: the axis permutation is
 * packed into one word (kx | ky << 2 | kz << 4) and S.z, which equals inv[kz], is not stored. */
struct RayAux {
    f3 inv;
    int k;
    float Sx, Sy;
};
WPT_D int auxKx(const RayAux& h) { return h.k & 3; }
WPT_D int auxKy(const RayAux& h) { return (h.k >> 2) & 3; }
WPT_D int auxKz(const RayAux& h) { return (h.k >> 4) & 3; }
/* SHEAR_ONLY: for triangle tests alone (the pdf of a light), which read the reciprocal of the direction's largest
 * component and nothing else of `inv`: that one division instead of three, the same bits */
template<bool SHEAR_ONLY = false> WPT_D RayAux rayAux(f3 dir)
{
    RayAux h;
    if (!SHEAR_ONLY)
        h.inv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    float ax = __builtin_fabsf(dir.x), ay = __builtin_fabsf(dir.y), az = __builtin_fabsf(dir.z);
    int kx, ky, kz;
    if (az >= ay && az >= ax)
        kz = 2;
    else if (ay >= ax)
        kz = 1;
    else
        kz = 0;
    kx = kz + 1;
    if (kx == 3)
        kx = 0;
    ky = kx + 1;
    if (ky == 3)
        ky = 0;
    if (comp(dir, kz) < 0.0f) {
        int tmp = kx;
        kx = ky;
        ky = tmp;
    }
    float invz;
    if (SHEAR_ONLY) {
        invz = 1.0f / comp(dir, kz);
        h.inv = mk3(invz, invz, invz);
    } else {
        invz = comp(h.inv, kz);
    }
    h.Sx = comp(dir, kx) * invz;
    h.Sy = comp(dir, ky) * invz;
    h.k = kx | (ky << 2) | (kz << 4);
    return h;
}

/* what survives of a triangle candidate: enough to rebuild the HitRecord later */
struct Candidate {
    uint32_t prim; /* 0xffffffff = no hit */
    float a, invDet, U, V, W; /* det itself is not kept: its sign is the sign of invDet */
};

/* Watertight test (hitable_triangle.hpp:189-271).  Returns true and fills c when accepted. */
WPT_D bool triangleTest(f3 v0, f3 v1, f3 v2, f3 org, const RayAux& h, float amin, float amax, Candidate& c)
{
    const f3 A = sub(v0, org);
    const f3 B = sub(v1, org);
    const f3 C = sub(v2, org);
    const int kx = auxKx(h), ky = auxKy(h), kz = auxKz(h);
    const float Sz = comp(h.inv, kz);
    const float Akz = comp(A, kz), Bkz = comp(B, kz), Ckz = comp(C, kz);
    const float Ax = comp(A, kx) - h.Sx * Akz;
    const float Ay = comp(A, ky) - h.Sy * Akz;
    const float Bx = comp(B, kx) - h.Sx * Bkz;
    const float By = comp(B, ky) - h.Sy * Bkz;
    const float Cx = comp(C, kx) - h.Sx * Ckz;
    const float Cy = comp(C, ky) - h.Sy * Ckz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (__builtin_fabsf(U) < k_ldeps || __builtin_fabsf(V) < k_ldeps || __builtin_fabsf(W) < k_ldeps) {
        double CxBy = (double)Cx * (double)By;
        double CyBx = (double)Cy * (double)Bx;
        U = (float)(CxBy - CyBx);
        double AxCy = (double)Ax * (double)Cy;
        double AyCx = (double)Ay * (double)Cx;
        V = (float)(AxCy - AyCx);
        double BxAy = (double)Bx * (double)Ay;
        double ByAx = (double)By * (double)Ax;
        W = (float)(BxAy - ByAx);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f))
        return false;
    float det = U + V + W;
    if (det == 0.0f)
        return false;
    const float Az = Sz * Akz;
    const float Bz = Sz * Bkz;
    const float Cz = Sz * Ckz;
    const float T = U * Az + V * Bz + W * Cz;
    const uint32_t sgn = wptm::float_to_bits(det) & 0x80000000u;
    const float Ts = wptm::bits_to_float(wptm::float_to_bits(T) ^ sgn);
    const float ds = wptm::bits_to_float(wptm::float_to_bits(det) ^ sgn);
    if (Ts < amin * ds || Ts > amax * ds)
        return false;
    const float invDet = 1.0f / det;
    c.a = invDet * T;
    c.invDet = invDet;
    c.U = U;
    c.V = V;
    c.W = W;
    return true;
}

/* ---- the test on corners stored in the ray's component order (the kernel with the scene and its rotated copies in LDS) ----
 * Unswapped, the reference's permutation (kx, ky, kz) = (kz + 1, kz + 2, kz) mod 3 is one of the three cyclic rotations of
 * (x, y, z); RAY_FLIP in RayAux::k says that the reference swaps kx and ky (dir[kz] < 0).  rayAuxRotated keeps the UNSWAPPED
 * shear constants Sx0 = dir[kz + 1] * invz, Sy0 = dir[kz + 2] * invz in Sx, Sy (the reference's swapped pair is (Sy0, Sx0): the
 * same two products), kx and ky unswapped in k. */
constexpr int RAY_FLIP = (int)0x80000000u; /* in RayAux::k: the sign bit, so that one AND makes the word triangleTestRotated takes */
template<bool SHEAR_ONLY = false> WPT_D RayAux rayAuxRotated(f3 dir)
{
    RayAux h;
    if (!SHEAR_ONLY)
        h.inv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    float ax = __builtin_fabsf(dir.x), ay = __builtin_fabsf(dir.y), az = __builtin_fabsf(dir.z);
    int kx, ky, kz;
    if (az >= ay && az >= ax)
        kz = 2;
    else if (ay >= ax)
        kz = 1;
    else
        kz = 0;
    kx = kz + 1;
    if (kx == 3)
        kx = 0;
    ky = kx + 1;
    if (ky == 3)
        ky = 0;
    const float dz = comp(dir, kz);
    float invz;
    if (SHEAR_ONLY) {
        invz = 1.0f / dz;
        h.inv = mk3(invz, invz, invz);
    } else {
        invz = comp(h.inv, kz);
    }
    h.Sx = comp(dir, kx) * invz;
    h.Sy = comp(dir, ky) * invz;
    h.k = kx | (ky << 2) | (kz << 4) | (dz < 0.0f ? RAY_FLIP : 0);
    return h;
}
/* a vector in the order of rotation kz: (v[kz + 1], v[kz + 2], v[kz]) */
WPT_D f3 rotated(f3 v, int kz)
{
    return kz == 2 ? v : (kz == 0 ? mk3(v.y, v.z, v.x) : mk3(v.z, v.x, v.y));
}

/* triangleTest on rotated values: c0, c1, c2 are the corners and org the ray's origin in the order of the ray's kz (rotated()),
 * Sx0, Sy0 the unswapped shear constants, Sz = inv[kz], flip = 0x80000000 where the reference swaps kx and ky, else 0.  No value
 * is selected by axis here.  Fills c with the reference's a, invDet, U, V, W bit for bit:
 *
 *  - Not swapped (flip = 0).  A.x, A.y, A.z below are the reference's A[kx], A[ky], A[kz] (the same subtraction of the same two
 *    numbers), Sx0, Sy0 its Sx, Sy, so p = Ax, q = Ay, and every later line is triangleTest's.
 *  - Swapped.  The reference's kx is kz + 2 and its Sx is Sy0, so its Ax is q and its Ay is p, for every corner: it computes
 *    U = Cq * Bp - Cp * Bq, V = Aq * Cp - Ap * Cq, W = Bq * Ap - Bp * Aq.  Here q carries the opposite sign (q' = -q, exactly: a sign
 *    bit), and the lines below compute U = Cp * Bq' - Cq' * Bp, V = Ap * Cq' - Aq' * Cp, W = Bp * Aq' - Bq' * Ap.  Every product is one
 *    p times one q', and IEEE multiplication is commutative and rounds symmetrically: Cp * Bq' = -(Cp * Bq) and Cq' * Bp = -(Cq * Bp)
 *    bit for bit.  So U = (-(Cp * Bq)) - (-(Cq * Bp)), which is the sum (Cq * Bp) + (-(Cp * Bq)) with its operands exchanged, and
 *    the reference's U is that same sum (x - y is x + (-y)); IEEE addition is commutative bit for bit, the sign of a zero sum
 *    included (equal products give +0 both ways, where negating the unswapped U afterwards would give -0, which invDet * U would
 *    carry into a hit record).  V and W alike.
 *  - The double-precision fall-back: the products of two floats are exact in double, negating a factor negates them exactly, the
 *    difference is the reference's sum with its operands exchanged, and the rounding to float is one rounding of one value.
 *  - |U|, |V|, |W| against k_ldeps, the sign tests, det, T (Az = Sz * A[kz], the same product) and the rest see the same numbers.
 * (Values that are NaN -- corners or origins beyond the float range's square root -- keep being NaN; which NaN is not covered.)
 * Checked over 10^8 random and adversarial cases on the CPU: tests/test_triangle_rotated.py. */
WPT_D bool triangleTestRotated(f3 c0, f3 c1, f3 c2, f3 org, float Sx0, float Sy0, float Sz, uint32_t flip, float amin, float amax, Candidate& c)
{
    const f3 A = sub(c0, org);
    const f3 B = sub(c1, org);
    const f3 C = sub(c2, org);
    const float Ax = A.x - Sx0 * A.z;
    const float Ay = wptm::bits_to_float(wptm::float_to_bits(A.y - Sy0 * A.z) ^ flip);
    const float Bx = B.x - Sx0 * B.z;
    const float By = wptm::bits_to_float(wptm::float_to_bits(B.y - Sy0 * B.z) ^ flip);
    const float Cx = C.x - Sx0 * C.z;
    const float Cy = wptm::bits_to_float(wptm::float_to_bits(C.y - Sy0 * C.z) ^ flip);
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (__builtin_fabsf(U) < k_ldeps || __builtin_fabsf(V) < k_ldeps || __builtin_fabsf(W) < k_ldeps) {
        double CxBy = (double)Cx * (double)By;
        double CyBx = (double)Cy * (double)Bx;
        U = (float)(CxBy - CyBx);
        double AxCy = (double)Ax * (double)Cy;
        double AyCx = (double)Ay * (double)Cx;
        V = (float)(AxCy - AyCx);
        double BxAy = (double)Bx * (double)Ay;
        double ByAx = (double)By * (double)Ax;
        W = (float)(BxAy - ByAx);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f))
        return false;
    float det = U + V + W;
    if (det == 0.0f)
        return false;
    const float Az = Sz * A.z;
    const float Bz = Sz * B.z;
    const float Cz = Sz * C.z;
    const float T = U * Az + V * Bz + W * Cz;
    const uint32_t sgn = wptm::float_to_bits(det) & 0x80000000u;
    const float Ts = wptm::bits_to_float(wptm::float_to_bits(T) ^ sgn);
    const float ds = wptm::bits_to_float(wptm::float_to_bits(det) ^ sgn);
    if (Ts < amin * ds || Ts > amax * ds)
        return false;
    const float invDet = 1.0f / det;
    c.a = invDet * T;
    c.invDet = invDet;
    c.U = U;
    c.V = V;
    c.W = W;
    return true;
}

/* triangleTestRotated in one straight run, for the leaf pass of the kernels with the scene in LDS: the same expressions in the same
 * order, but no early return -- every lane evaluates det, T, the range condition, 1 / det and a, and the three rejections are
 * combined without short circuit.  A wave leaves a region of the branching form only when all its lanes fail there, which a leaf
 * pass of a dozen lanes against wall-sized triangles rarely does, while each region costs it scalar instructions, a wait for a
 * comparison to reach the scalar side and a branch ("The leaf pass in one straight run").  The comparisons
 * are the reference's own, not their negated opposites: with a NaN all of them are false and the case is accepted, as there.
 * c is written in every case; where the result is false its values are not the branching form's (which leaves c alone) and may be
 * infinite or NaN -- nothing traps -- so the caller selects by the result.  The double-precision fall-back is rare and long and
 * keeps its branch.  Held to triangleTestRotated bit for bit in tests/test_triangle_straight.py. */
WPT_D bool triangleTestRotatedStraight(f3 c0, f3 c1, f3 c2, f3 org, float Sx0, float Sy0, float Sz, uint32_t flip, float amin, float amax, Candidate& c)
{
    const f3 A = sub(c0, org);
    const f3 B = sub(c1, org);
    const f3 C = sub(c2, org);
    const float Ax = A.x - Sx0 * A.z;
    const float Ay = wptm::bits_to_float(wptm::float_to_bits(A.y - Sy0 * A.z) ^ flip);
    const float Bx = B.x - Sx0 * B.z;
    const float By = wptm::bits_to_float(wptm::float_to_bits(B.y - Sy0 * B.z) ^ flip);
    const float Cx = C.x - Sx0 * C.z;
    const float Cy = wptm::bits_to_float(wptm::float_to_bits(C.y - Sy0 * C.z) ^ flip);
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (__builtin_expect(__builtin_fabsf(U) < k_ldeps || __builtin_fabsf(V) < k_ldeps || __builtin_fabsf(W) < k_ldeps, 0)) {
        double CxBy = (double)Cx * (double)By;
        double CyBx = (double)Cy * (double)Bx;
        U = (float)(CxBy - CyBx);
        double AxCy = (double)Ax * (double)Cy;
        double AyCx = (double)Ay * (double)Cx;
        V = (float)(AxCy - AyCx);
        double BxAy = (double)Bx * (double)Ay;
        double ByAx = (double)By * (double)Ax;
        W = (float)(BxAy - ByAx);
    }
    const int mixedSigns = ((U < 0.0f) | (V < 0.0f) | (W < 0.0f)) & ((U > 0.0f) | (V > 0.0f) | (W > 0.0f));
    const float det = U + V + W;
    const int zeroDet = det == 0.0f;
    const float Az = Sz * A.z;
    const float Bz = Sz * B.z;
    const float Cz = Sz * C.z;
    const float T = U * Az + V * Bz + W * Cz;
    const uint32_t sgn = wptm::float_to_bits(det) & 0x80000000u;
    const float Ts = wptm::bits_to_float(wptm::float_to_bits(T) ^ sgn);
    const float ds = wptm::bits_to_float(wptm::float_to_bits(det) ^ sgn);
    const int outOfRange = (Ts < amin * ds) | (Ts > amax * ds);
    const float invDet = 1.0f / det;
    c.a = invDet * T;
    c.invDet = invDet;
    c.U = U;
    c.V = V;
    c.W = W;
    return !(mixedSigns | zeroDet | outOfRange);
}

} /* namespace wptd */

#endif
