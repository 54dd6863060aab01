/*
 * wpt_capi_selftest.hip -- the test hooks wpt_selftest_* (not in include/wurblpt_hip.h; the tests and the oracle declare them)
 * and their kernels: the arithmetic and the intersection tests as the path-tracing kernels evaluate them, one lane per case.
 */
#include <cstring>

#include "wpt_capi_common.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

namespace {

/* Bit-parity self test of the arithmetic the kernel relies on: ops 0..5 are the
 * transcendentals of wpt_math.h, 6 = IEEE division, 7 = IEEE square root, 10 acos, 11 atan2(x, 1), 12 float(2 * asin(double)),
 * 13 / 14 the sine / cosine of sincosf_(x), 15 / 16 the x / y of the sampler's inUnitDisk(x, y). */
__global__ void wpt_selftest_kernel(int op, int n, const float* a, const float* b, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float x = a[i], y = b[i], r;
    switch (op) {
    case 0: r = wptm::sinf_(x); break;
    case 1: r = wptm::cosf_(x); break;
    case 2: r = wptm::expf_(x); break;
    case 3: r = wptm::powf_(x, y); break;
    case 4: r = wptm::asinf_(x); break;
    case 5: r = wptm::atan2f_(x, y); break;
    case 6: r = x / y; break;
    case 7: r = __builtin_sqrtf(x); break;
    case 8: r = x * y + x; break; /* must stay unfused */
    case 10: r = wptm::acosf_(x); break;
    case 11: r = wptm::atan2f_(x, 1.0f); break;
    case 12: r = (float)(2.0 * wptm::asin_d((double)x)); break;
    case 13:
    case 14: {
        float s, c;
        wptm::sincosf_(x, &s, &c);
        r = op == 13 ? s : c;
        break;
    }
    case 15:
    case 16: {
        f2 u;
        u.x = x;
        u.y = y;
        const f2 d = inUnitDisk(u);
        r = op == 15 ? d.x : d.y;
        break;
    }
    default: r = 1.0f / x; break;
    }
    out[i] = r;
}

/* AABB::mayHit as the kernels evaluate it; same argument layout as the oracle's probe:
 * boxes lo(3) hi(3); rays origin(3) dir(3) amin amax */
__global__ void wpt_selftest_aabb_kernel(int n, const float* boxes, const float* rays, int32_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const RayAux h = rayAux(ld3(rays + 8 * i + 3));
    out[i] = boxTest(ld3(boxes + 6 * i), ld3(boxes + 6 * i + 3), ld3(rays + 8 * i), h.inv, rays[8 * i + 6], rays[8 * i + 7]) ? 1 : 0;
}

/* The watertight triangle test as the kernels call it, one lane per case.  cases: v0 v1 v2 origin direction amin amax (17 floats);
 * out: 8 words: accepted, the bits of a, invDet, U, V, W (zero when rejected), RayAux::k, one spare.  form 0: rayAux +
 * triangleTest (the walks that select by axis); 1: rayAuxRotated + rotated() + triangleTestRotated with Sz = inv[kz] (the walk on
 * rotated corner copies); 2, 3: the SHEAR_ONLY variants of the light-pdf loop, Sz = inv.x (hotSpotPdfValue, hotSpotPdfValueRotated);
 * 4: form 1's arguments through triangleTestRotatedStraight (the leaf pass of the rotated kernels with the scene in LDS). */
__global__ void wpt_selftest_triangle_kernel(int form, int n, const float* cases, uint32_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float* in = cases + 17 * (size_t)i;
    const f3 v0 = ld3(in), v1 = ld3(in + 3), v2 = ld3(in + 6), org = ld3(in + 9), dir = ld3(in + 12);
    const float amin = in[15], amax = in[16];
    Candidate c;
    c.prim = 0;
    c.a = c.invDet = c.U = c.V = c.W = 0.0f;
    bool accepted;
    int k;
    if (form == 0) {
        const RayAux h = rayAux(dir);
        k = h.k;
        accepted = triangleTest(v0, v1, v2, org, h, amin, amax, c);
    } else if (form == 1) {
        const RayAux h = rayAuxRotated(dir);
        const int kz = auxKz(h);
        k = h.k;
        accepted = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), h.Sx, h.Sy, comp(h.inv, kz),
                (uint32_t)h.k & (uint32_t)RAY_FLIP, amin, amax, c);
    } else if (form == 2) {
        const RayAux h = rayAux<true>(dir);
        k = h.k;
        accepted = triangleTest(v0, v1, v2, org, h, amin, amax, c);
    } else if (form == 3) {
        const RayAux h = rayAuxRotated<true>(dir);
        const int kz = auxKz(h);
        k = h.k;
        accepted = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), h.Sx, h.Sy, h.inv.x,
                (uint32_t)h.k & (uint32_t)RAY_FLIP, amin, amax, c);
    } else {
        const RayAux h = rayAuxRotated(dir);
        const int kz = auxKz(h);
        k = h.k;
        accepted = triangleTestRotatedStraight(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), h.Sx, h.Sy, comp(h.inv, kz),
                (uint32_t)h.k & (uint32_t)RAY_FLIP, amin, amax, c);
    }
    uint32_t* o = out + 8 * (size_t)i;
    o[0] = accepted ? 1u : 0u;
    o[1] = accepted ? __float_as_uint(c.a) : 0u;
    o[2] = accepted ? __float_as_uint(c.invDet) : 0u;
    o[3] = accepted ? __float_as_uint(c.U) : 0u;
    o[4] = accepted ? __float_as_uint(c.V) : 0u;
    o[5] = accepted ? __float_as_uint(c.W) : 0u;
    o[6] = (uint32_t)k;
    o[7] = 0u;
}

/* RayIntersectionHelper as the kernels make it; dirs: 3 floats per ray; out: 18 floats per ray, twice inv (3), kx ky kz (as
 * floats), S (3) with S.z = inv[kz]: first from rayAux, then from rayAuxRotated with the swap it keeps as a flag applied */
__global__ void wpt_selftest_rayaux_kernel(int n, const float* dirs, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const f3 dir = ld3(dirs + 3 * (size_t)i);
    float* o = out + 18 * (size_t)i;
    const RayAux h = rayAux(dir);
    o[0] = h.inv.x; o[1] = h.inv.y; o[2] = h.inv.z;
    o[3] = (float)auxKx(h); o[4] = (float)auxKy(h); o[5] = (float)auxKz(h);
    o[6] = h.Sx; o[7] = h.Sy; o[8] = comp(h.inv, auxKz(h));
    const RayAux r = rayAuxRotated(dir);
    const bool flip = ((uint32_t)r.k & (uint32_t)RAY_FLIP) != 0;
    o[9] = r.inv.x; o[10] = r.inv.y; o[11] = r.inv.z;
    o[12] = (float)(flip ? auxKy(r) : auxKx(r)); o[13] = (float)(flip ? auxKx(r) : auxKy(r)); o[14] = (float)auxKz(r);
    o[15] = flip ? r.Sy : r.Sx; o[16] = flip ? r.Sx : r.Sy; o[17] = comp(r.inv, auxKz(r));
}

/* HitableSphere::hit's candidate part as the kernels evaluate it; spheres: centre (3) radius; rays: origin(3) dir(3) amin amax;
 * out: accepted, a (zero when rejected) */
__global__ void wpt_selftest_sphere_kernel(int n, const float* spheres, const float* rays, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    wpt_sphere sp;
    memset(&sp, 0, sizeof(sp));
    sp.center[0] = spheres[4 * (size_t)i];
    sp.center[1] = spheres[4 * (size_t)i + 1];
    sp.center[2] = spheres[4 * (size_t)i + 2];
    sp.radius = spheres[4 * (size_t)i + 3];
    const float* r = rays + 8 * (size_t)i;
    float a = 0.0f;
    const bool accepted = sphereTest(sp, ld3(r), ld3(r + 3), r[6], r[7], a);
    out[2 * (size_t)i] = accepted ? 1.0f : 0.0f;
    out[2 * (size_t)i + 1] = accepted ? a : 0.0f;
}

} /* namespace */

extern "C" {

/* behind a hook's launch: its error, then the device's once the kernel has run */
static wpt_status launched()
{
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

/* test hook: evaluates one arithmetic primitive on the device for n inputs (device pointers) */
wpt_status wpt_selftest_aabb(int n, const float* boxes_device, const float* rays_device, int32_t* out_device)
{
    if (n <= 0 || !boxes_device || !rays_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_aabb_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, boxes_device, rays_device, out_device);
    return launched();
}

/* test hooks: the triangle test in the five forms the kernels call it in, the ray's constants, the sphere test, and the closest
 * hit of a scene with its finished record (kernels above and in wpt_k_groundtruth.hip; all pointers are device pointers) */
wpt_status wpt_selftest_triangle(int form, int n, const float* cases_device, uint32_t* out_device)
{
    if (form < 0 || form > 4 || n <= 0 || !cases_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_triangle_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, form, n, cases_device, out_device);
    return launched();
}

wpt_status wpt_selftest_rayaux(int n, const float* dirs_device, float* out_device)
{
    if (n <= 0 || !dirs_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_rayaux_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dirs_device, out_device);
    return launched();
}

wpt_status wpt_selftest_sphere(int n, const float* spheres_device, const float* rays_device, float* out_device)
{
    if (n <= 0 || !spheres_device || !rays_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_sphere_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, spheres_device, rays_device, out_device);
    return launched();
}

wpt_status wpt_selftest_hits(wpt_scene* scene, int n, const float* rays8_device, float* out15_device)
{
    if (!scene || n <= 0 || !rays8_device || !out15_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    launchSelftestHits(scene->view, n, rays8_device, out15_device, nullptr);
    return launched();
}

/* the same for rays and records in host memory (a program without the HIP runtime of its own: oracle/pin_render.cpp) */
wpt_status wpt_selftest_hits_host(wpt_scene* scene, int n, const float* rays8_host, float* out15_host)
{
    if (!scene || n <= 0 || !rays8_host || !out15_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    StagedBlock rays, out;
    hipError_t e = rays.allocate(size_t(n) * 8 * sizeof(float));
    if (e == hipSuccess)
        e = out.allocate(size_t(n) * 15 * sizeof(float));
    if (e == hipSuccess)
        e = rays.upload(rays8_host);
    WPT_TRY(hipStatus("self test", e));
    WPT_TRY(wpt_selftest_hits(scene, n, static_cast<const float*>(rays.device), static_cast<float*>(out.device)));
    return hipStatus("self test", out.download(out15_host));
}

wpt_status wpt_selftest_math(int op, int n, const float* a_device, const float* b_device, float* out_device)
{
    if (n <= 0)
        return WPT_OK;
    hipLaunchKernelGGL(wpt_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, a_device, b_device, out_device);
    return launched();
}

} /* extern "C" */
