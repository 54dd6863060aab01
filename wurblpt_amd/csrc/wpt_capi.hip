/*
 * wpt_capi.hip -- the C ABI of include/wurblpt_hip.h: scene upload, kernel selection and launch.  What an uploaded scene looks
 * like -- validation, the stackless node form and its storage order, the wide form, the triangles' order, the texel and
 * measured-BRDF pools, the environment's tables -- is decided by the pure host functions of wpt_scene_layout.h; wpt_scene_upload
 * copies what they return and runs the three kernels that finish a scene on the device.  Which kernel renders a launch is
 * wpt_kernel_table.h, which passes wpt_launch_plan.h.  The kernel itself is in wpt_pathtrace.inc.h.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/wurblpt_hip.h"
#include "wpt_pathtrace.inc.h"
#include "wpt_kernel_table.h"
#include "wpt_launch_plan.h"
#include "wpt_scene_layout.h"
#include "wpt_bypass.h"
#include "wpt_leaf_words.h"
#include "wpt_wavefront.inc.h"
#include "wpt_postproc.h"
#include "wpt_lightmix.h"
#include "wpt_denoise_launch.h"
#include "wpt_firsthit_launch.h"
#include "wpt_image_ops_launch.h"
#include "wpt_streams_launch.h"
#include "wpt_progress.h"
#include "wpt_progress_state.h"

using namespace wptd;
using namespace wptk;

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
 * rotated corner copies); 2, 3: the SHEAR_ONLY variants of the light-pdf loop, Sz = inv.x (hotSpotPdfValue, hotSpotPdfValueRotated). */
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
    } else {
        const RayAux h = rayAuxRotated<true>(dir);
        const int kz = auxKz(h);
        k = h.k;
        accepted = triangleTestRotated(rotated(v0, kz), rotated(v1, kz), rotated(v2, kz), rotated(org, kz), h.Sx, h.Sy, h.inv.x,
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

/* per-bin importance of the environment map (envmap.hpp:128-140) */
__global__ void wpt_env_importance_kernel(SceneView sv, int N, float* importance)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * N)
        return;
    int x = i % N, y = i / N;
    f2 uv;
    uv.y = ((float)y + 0.5f) / (float)N;
    uv.x = ((float)x + 0.5f) / (float)N;
    f4 L = envL(sv, envInvM(uv));
    importance[i] = L.x + L.y + L.z + L.w;
}

/* per triangle hot spot: what its pdf needs of the corners alone (wpt_blocks.h hotSpotFace; the corners are the world-space
 * positions the walk tests, tri_geom) */
__global__ void wpt_hotspot_face_kernel(SceneView sv, float4* face)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sv.hotspotCount)
        return;
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sv.hotspots[i].kind != WPT_HOTSPOT_SPHERE) {
        const uint32_t p = sv.hotspots[i].prim;
        const float4 g0 = sv.triGeom[3 * p], g1 = sv.triGeom[3 * p + 1], g2 = sv.triGeom[3 * p + 2];
        f = wptk::hotSpotFace(mk3(g0.x, g0.y, g0.z), mk3(g1.x, g1.y, g1.z), mk3(g2.x, g2.y, g2.z));
    }
    face[i] = f;
}

/* decodes one image texture into the RGBA float4 pool (see imageTexelDecode) */
__global__ void wpt_expand_texels_kernel(const uint8_t* pool, const wpt_texture t, float4* out)
{
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= size_t(t.width) * t.height)
        return;
    const f4 v = imageTexelDecode(pool, t, i % t.width, i / t.width);
    out[i] = make_float4(v.x, v.y, v.z, v.w);
}

/* ---- output side: one thread per pixel (wpt_postproc.h) ---- */
struct DevicePow {
    static __device__ __forceinline__ float pow(float x, float y) { return wptm::powf_(x, y); }
};
__global__ void wpt_postproc_kernel(int op, const float* in, void* out, uint64_t pixels, float a, float b, uint32_t* maxBits)
{
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= pixels)
        return;
    wptpp::V3 rgb;
    rgb.x = in[3 * i];
    rgb.y = in[3 * i + 1];
    rgb.z = in[3 * i + 2];
    if (op == 0) {
        uint8_t* o = static_cast<uint8_t*>(out) + 3 * i;
        o[0] = wptpp::toSrgbByte<DevicePow>(rgb.x);
        o[1] = wptpp::toSrgbByte<DevicePow>(rgb.y);
        o[2] = wptpp::toSrgbByte<DevicePow>(rgb.z);
    } else if (op == 3) {
        /* maximum of non-negative floats = maximum of their bit patterns; NaN and negative values never win,
         * as in the sequential `if (y > lum)` starting from 0 */
        const float y = wptpp::luminance(rgb);
        if (y > 0.0f)
            atomicMax(maxBits, __float_as_uint(y));
    } else {
        const wptpp::V3 r = op == 1 ? wptpp::uniformRationalQuantization(rgb, a, b) : wptpp::scaleLuminance(rgb, a, b);
        float* o = static_cast<float*>(out) + 3 * i;
        o[0] = r.x;
        o[1] = r.y;
        o[2] = r.z;
    }
}

/* ---- host side of the C ABI ---- */

thread_local std::string g_error;

wpt_status fail(wpt_status s, const std::string& msg)
{
    g_error = msg;
    return s;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(WPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)
#define WPT_TRY(expr)                                                                              \
    do {                                                                                           \
        const wpt_status s_ = (expr);                                                              \
        if (s_ != WPT_OK)                                                                          \
            return s_;                                                                             \
    } while (0)

} /* namespace */

struct wpt_scene {
    int device;
    SceneView view;
    uint32_t features;
    uint32_t nodeCount, triCount;
    uint32_t foldedLinks; /* wpt_scene_folded_links */
    /* a scene that fits LDS: the link words of its tree's copy there (wpt_bypass.h, Plan), three arrays of 2 * nodeCount + 4
     * words one behind the other -- plain, folded, bypass -- and the inner nodes the last one leaves out; else NULL */
    uint32_t* ldsLinks = nullptr;
    /* ... and behind them the same three sets for the kernels with rotated corner copies (wpt_leaf_words.h: leaf words that say
     * where the corners lie, and per triangle its leaf's skip link), wptw::leafWordsSize words each.  leafOneToOne: every
     * triangle has exactly one leaf, so the leaf pass of those kernels takes its links from the corner records */
    bool leafOneToOne = false;
    uint32_t bypassedNodes = 0; /* wpt_scene_bypassed_nodes */
    uint32_t animationCount;
    std::vector<void*> allocations;
    int cuCount;
    std::vector<float> envM, envMcs;
    std::vector<int32_t> envMs;
};

namespace {

uint32_t g_threadsPerGroup = WG;
uint32_t g_variant = 0;
uint32_t g_leaveEighths = 0; /* 0 = default: chosen per scene size (single-role kernel) / patience 8 rounds (ray-pool kernel) */
uint32_t g_heavyMin = 0; /* 0 = chosen per scene size at launch */
uint32_t g_leafBias = 0;
/* what the process's most recent render call ran: kernel launches it took for its pixels (wpt_last_render_passes) and which
 * kernel family (wpt_kernel_name).  Process-wide, so that a caller whose worker threads render (MPICoordinator, bench.py's
 * block queue) reads on its main thread what the workers ran. */
std::atomic<uint32_t> g_lastPasses{1};
std::atomic<const char*> g_kernelName{nullptr};
std::atomic<const char*> g_kernelForm{""}; /* wpt_kernel_form */
uint32_t g_topNodes = 65536; /* nodes of a large tree that are stored level by level in front (wpt_set_top_nodes) */
unsigned long long* g_schedStats = nullptr;
/* wpt_set_wavefront: 0 = the library decides, 1 = wavefront wherever it exists, 2 = never; launch geometry (0 = defaults) */
uint32_t g_wfMode = 0;
wptk::WfConfig g_wfConfig = { 0, 0, 0, 1, 0, 0, 0, 0, 0 };
/* wpt_set_walk: WPT_WALK_* bits */
uint32_t g_walk = 0;
/* wpt_set_bypass: how scenes uploaded from now on choose the nodes their walk leaves out (wpt_bypass.h) */
uint32_t g_bypassMode = wptb::MODE_MODEL;
/* wpt_set_slices: 0 = wpt_slices_plan, 1 = never, 2 .. 15 = that many units; WPT_SLICES_DECLINE_ODD beside it */
uint32_t g_slices = 0;
/* the two counters of the sliced kernels (wpt_last_slice_stats), one pair per device, allocated at a device's first sliced
 * launch and kept; g_lastSliceStats: the pair the most recent render call's kernel adds to, or NULL if it was not sliced */
constexpr int SLICE_STATS_DEVICES = 64;
std::atomic<unsigned long long*> g_sliceStats[SLICE_STATS_DEVICES];
std::atomic<unsigned long long*> g_lastSliceStats{nullptr};
static_assert(wptk::PLAN_WG == uint32_t(WG) && wptk::PLAN_SLICE_SLOT_MAX == wptk::SLICE_SLOT_MASK && wptk::SLICE_UNITS_TARGET <= wptk::SLICE_UNITS_MAX
        && wptk::PLAN_FRAME == wptk::SENSOR_FRAME && wptk::PLAN_VIEWS == wptk::SENSOR_VIEWS && wptk::PLAN_ADAPTIVE == wptk::SENSOR_ADAPTIVE
        && wptk::PLAN_SENSORS == wptk::SENSOR_COUNT, "wpt_launch_plan.h restates the kernels' constants and the sensors");
static_assert(wptl::NODE_CHILD == NODE_CHILD && wptl::NODE_INDEX_MASK == NODE_INDEX_MASK && wptl::PRIM_SPHERE == PRIM_SPHERE && wptl::WIDE_STACK == WIDE_STACK
        && wptl::WIDE_NONE == WIDE_NONE && wptl::LDS_SCENE_MAX_BYTES == LDS_SCENE_MAX_BYTES, "wpt_scene_layout.h restates the kernels' node words and limits");

static_assert(wptw::LEAF_NODE_SHIFT == wptk::LEAF_NODE_SHIFT && wptw::LEAF_NODE_MAX == wptk::LEAF_NODE_MAX && wptw::LEAF_CORNER_MASK == wptk::LEAF_CORNER_MASK
        && LDS_SCENE_MAX_BYTES / 32 <= wptw::LEAF_NODE_MAX && LDS_SCENE_MAX_BYTES / 16 <= wptw::LEAF_CORNER_MASK,
        "wpt_leaf_words.h restates the rotated kernels' leaf word, which has room for every tree that fits LDS");

/* What the process's most recent render call ran, all of it at once: every path that renders stores it here and nowhere else
 * (the wavefront form and the stages of a session too).  sliceStats: the counters a sliced launch adds to, else NULL. */
void recordLaunch(const char* name, const char* form, uint32_t passes, unsigned long long* sliceStats)
{
    g_kernelName.store(name, std::memory_order_relaxed);
    g_kernelForm.store(form, std::memory_order_relaxed);
    g_lastPasses.store(passes, std::memory_order_relaxed);
    g_lastSliceStats.store(sliceStats, std::memory_order_relaxed);
}

/* wpt_kernel_form of a launch: "rotated corners" for that form of the kernel with the scene in LDS -- with ", leaf links from
 * the nodes" where the scene's tree is not one leaf per triangle and the leaf pass reads the leaf's node (wpt_leaf_words.h) --
 * and ", sliced xU" behind it for a launch that hands its pixels out in U > 1 units */
const char* kernelForm(bool rotated, uint32_t units = 0, bool leafLinksFromNodes = false)
{
    static const std::vector<std::string> forms = [] {
        std::vector<std::string> f;
        for (int r = 0; r < 3; r++)
            for (uint32_t u = 0; u <= wptk::SLICE_UNITS_MAX; u++)
                f.push_back(std::string(r ? "rotated corners" : "") + (r == 2 ? ", leaf links from the nodes" : "")
                        + (u > 1 ? ", sliced x" + std::to_string(u) : std::string()));
        return f;
    }();
    return forms[(rotated ? (leafLinksFromNodes ? 2 : 1) * (wptk::SLICE_UNITS_MAX + 1) : 0) + (units <= wptk::SLICE_UNITS_MAX ? units : 0)].c_str();
}

/* the kernel table's row for an instantiation; there is no launch without one */
wpt_status lookupKernel(uint32_t features, bool count, bool ldsScene, bool wide, const wptk::KernelEntry** entry)
{
    *entry = wptk::findKernel(features, count, ldsScene, wide);
    if (!*entry)
        return fail(WPT_ERR_UNSUPPORTED, "the library has no kernel wpt_pathtrace<F = " + std::to_string(features) + ", COUNT = " + std::to_string(count)
                + ", LDSSCENE = " + std::to_string(ldsScene) + ", WIDE = " + std::to_string(wide) + ">");
    return WPT_OK;
}

unsigned long long* sliceStatsOfCurrentDevice()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SLICE_STATS_DEVICES)
        return nullptr;
    unsigned long long* p = g_sliceStats[dev].load(std::memory_order_acquire);
    if (!p) {
        if (hipMalloc(reinterpret_cast<void**>(&p), 2 * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        unsigned long long* expected = nullptr;
        if (!g_sliceStats[dev].compare_exchange_strong(expected, p, std::memory_order_acq_rel)) {
            (void)hipFree(p);
            p = expected;
        }
    }
    return p;
}

template<typename T> wpt_status uploadArray(wpt_scene* s, const T* src, size_t count, const T** dst)
{
    *dst = nullptr;
    size_t bytes = count * sizeof(T);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes > 0 ? bytes : 16);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    s->allocations.push_back(p);
    if (bytes > 0)
        HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return WPT_OK;
}

wpt_status uploadQuads(wpt_scene* s, const std::vector<wptl::Quad>& quads, const float4** dst)
{
    static_assert(sizeof(wptl::Quad) == sizeof(float4), "the layout's quadwords are the device's");
    return uploadArray(s, reinterpret_cast<const float4*>(quads.data()), quads.size(), dst);
}

wpt_status layoutStatus(const wptl::Status& st)
{
    return st.code == WPT_OK ? WPT_OK : fail(st.code, st.message);
}

wpt_status hipStatus(hipError_t e, const char* what)
{
    if (e == hipSuccess)
        return WPT_OK;
    return fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

/* what wpt_scene_upload owns until its last line, and its temporary device buffers: freed on every way out */
struct SceneFree {
    void operator()(wpt_scene* s) const { wpt_scene_free(s); }
};
struct DeviceFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
using DeviceTemp = std::unique_ptr<void, DeviceFree>;

wpt_status deviceTemp(size_t bytes, const char* what, DeviceTemp* mem)
{
    void* p = nullptr;
    WPT_TRY(hipStatus(hipMalloc(&p, bytes > 0 ? bytes : 16), what));
    mem->reset(p);
    return WPT_OK;
}

/* device memory that lives as long as the scene */
wpt_status sceneAlloc(wpt_scene* s, size_t bytes, const char* what, void** p)
{
    WPT_TRY(hipStatus(hipMalloc(p, bytes > 0 ? bytes : 16), what));
    s->allocations.push_back(*p);
    return WPT_OK;
}

/* the pool of decoded texels that devTex indexes (wptl::texelOffsets), filled from the caller's raw pool by one launch per image */
wpt_status decodeTexels(wpt_scene* s, const wpt_scene_desc* desc, const std::vector<wpt_texture>& devTex, size_t texelCount)
{
    void* pool = nullptr;
    WPT_TRY(sceneAlloc(s, texelCount * sizeof(float4), "hipMalloc for the decoded texel pool", &pool));
    s->view.texels4 = static_cast<const float4*>(pool);
    if (texelCount == 0)
        return WPT_OK;
    DeviceTemp raw;
    WPT_TRY(deviceTemp(desc->texel_bytes, "texel decode", &raw));
    WPT_TRY(hipStatus(hipMemcpy(raw.get(), desc->texels, desc->texel_bytes, hipMemcpyHostToDevice), "texel decode"));
    for (uint32_t i = 0; i < desc->texture_count; i++) {
        const wpt_texture& t = desc->textures[i];
        if (t.type != WPT_TEX_IMAGE)
            continue;
        const size_t n = size_t(t.width) * t.height;
        hipLaunchKernelGGL(wpt_expand_texels_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, 0,
                static_cast<const uint8_t*>(raw.get()), t, static_cast<float4*>(pool) + devTex[i].texel_offset);
        WPT_TRY(hipStatus(hipGetLastError(), "texel decode"));
    }
    return hipStatus(hipDeviceSynchronize(), "texel decode");
}

/* SceneView::hotspotFace from the view's hot spots and triangles as uploaded */
wpt_status hotspotFaces(wpt_scene* s)
{
    void* face = nullptr;
    WPT_TRY(sceneAlloc(s, size_t(s->view.hotspotCount) * sizeof(float4), "hot spot faces", &face));
    hipLaunchKernelGGL(wpt_hotspot_face_kernel, dim3((s->view.hotspotCount + 255) / 256), dim3(256), 0, 0, s->view, static_cast<float4*>(face));
    WPT_TRY(hipStatus(hipDeviceSynchronize(), "hot spot faces"));
    s->view.hotspotFace = static_cast<const float4*>(face);
    return WPT_OK;
}

/* per-bin importance of the environment (envmap.hpp:128-140) from the device's own L() over the view as it is */
wpt_status envImportance(const SceneView& view, int N, std::vector<float>* importance)
{
    const size_t bins = size_t(N) * N;
    DeviceTemp dImp;
    WPT_TRY(deviceTemp(bins * sizeof(float), "hipMalloc for the importance map", &dImp));
    hipLaunchKernelGGL(wpt_env_importance_kernel, dim3((bins + 255) / 256), dim3(256), 0, 0, view, N, static_cast<float*>(dImp.get()));
    importance->resize(bins);
    return hipStatus(hipMemcpy(importance->data(), dImp.get(), bins * sizeof(float), hipMemcpyDeviceToHost), "importance map");
}

uint32_t sceneFeatures(const wpt_scene_desc* d)
{
    uint32_t f = 0;
    for (uint32_t i = 0; i < d->material_count; i++) {
        const wpt_material& m = d->materials[i];
        if (m.type == WPT_MAT_MODPHONG)
            f |= FEAT_MODPHONG;
        if (m.type == WPT_MAT_TWOSIDED)
            f |= FEAT_TWOSIDED;
        if (m.type == WPT_MAT_GGX)
            f |= FEAT_GGX;
        if (m.type == WPT_MAT_GLASS || m.type == WPT_MAT_MIRROR)
            f |= FEAT_GLASS;
        if (m.type == WPT_MAT_LIGHT_SPOT)
            f |= FEAT_SPOT;
        bool tex = m.normal_tex >= 0;
        if (m.type != WPT_MAT_TWOSIDED)
            for (int k = 0; k < 5; k++)
                tex = tex || m.tex[k] >= 0;
        if (tex)
            f |= FEAT_TEXTURES;
    }
    if (d->envmap.type != WPT_ENV_NONE)
        f |= FEAT_ENVMAP | FEAT_TEXTURES;
    if (d->sphere_count > 0)
        f |= FEAT_SPHERES;
    for (uint32_t i = 0; i < d->material_count; i++)
        if (d->materials[i].type == WPT_MAT_RGL)
            f |= FEAT_RGL;
    for (uint32_t i = 0; i < d->instance_count; i++)
        if (d->instances[i].animation >= 0)
            f |= FEAT_ANIM;
    for (uint32_t i = 0; i < d->sphere_count; i++)
        if (d->spheres[i].animation >= 0)
            f |= FEAT_ANIM;
    return f;
}

/* wptl::validate, its message kept for wpt_last_error */
wpt_status validate(const wpt_scene_desc* d)
{
    return layoutStatus(wptl::validate(d));
}


} /* namespace */

extern "C" {

int wpt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        g_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return 0;
    }
    return n;
}

wpt_status wpt_select_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return WPT_OK;
}

wpt_status wpt_current_device(int* device)
{
    if (!device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "device is NULL");
    HIP_TRY(hipGetDevice(device));
    return WPT_OK;
}

/* Lay out, copy, release: one array at a time (wpt_scene_layout.h says what each looks like; DESIGN.md section 3 has the table),
 * then the three kernels that finish the scene on the device, each reading the view as it is at that moment. */
wpt_status wpt_scene_upload(const wpt_scene_desc* desc, wpt_scene** out_scene)
{
    if (!out_scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "out_scene is NULL");
    *out_scene = nullptr;
    WPT_TRY(validate(desc));
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; the path tracer has no CPU fallback");
    /* the process's hooks, read once: what the scene looks like on the device is a function of the description and these two */
    const uint32_t walk = g_walk, topNodes = g_topNodes;
    std::unique_ptr<wpt_scene, SceneFree> owner(new wpt_scene);
    wpt_scene* s = owner.get();
    SceneView& view = s->view;
    HIP_TRY(hipGetDevice(&s->device));
    s->features = sceneFeatures(desc);
    s->nodeCount = desc->node_count;
    s->triCount = desc->tri_count;
    memset(&view, 0, sizeof(view));
    const std::vector<uint32_t> triNew = wptl::triangleOrder(desc, (walk & WPT_WALK_TRIANGLES_AS_GIVEN) != 0);
    const bool fitsLds = size_t(desc->node_count) * 32 + size_t(desc->tri_count) * 48 <= LDS_SCENE_MAX_BYTES;
    std::vector<uint32_t> ldsNodes; /* the device nodes of a tree that fits LDS, kept for its link words below */
    {
        wptl::DeviceNodes nodes;
        WPT_TRY(layoutStatus(wptl::deviceNodes(desc, triNew, topNodes, &nodes)));
        view.nodeCount = desc->node_count;
        view.boxesMayBeNan = nodes.boxesMayBeNan;
        WPT_TRY(uploadQuads(s, nodes.quads, &view.nodes));
        s->foldedLinks = 0;
        if (fitsLds) { /* the trees that are walked from LDS */
            s->foldedLinks = wptl::countFoldedLinks(reinterpret_cast<const uint32_t*>(nodes.quads.data()), desc->node_count, nullptr);
            ldsNodes.resize(size_t(desc->node_count) * 8);
            memcpy(ldsNodes.data(), nodes.quads.data(), ldsNodes.size() * 4);
        }
    }
    if (walk & WPT_WALK_WIDE) {
        const std::vector<wptl::Quad> wide = wptl::wideNodes(desc, triNew);
        if (!wide.empty()) /* a tree without a wide form is walked as it is */
            WPT_TRY(uploadQuads(s, wide, &view.wideNodes));
    }
    {
        const std::vector<wpt_tri_geom> g = wptl::permuted(desc->tri_geom, triNew);
        WPT_TRY(uploadArray(s, reinterpret_cast<const float4*>(g.data()), size_t(desc->tri_count) * 3, &view.triGeom));
        if (fitsLds) {
            /* the link words of the tree's copy in LDS, computed once per scene: the exact ones, plain and folded, and the
             * ones that go round the nodes the plan leaves out (wpt_bypass.h) */
            const wptb::Plan plan = wptb::plan(ldsNodes.data(), desc->node_count, g.data(), desc->tri_count, g_bypassMode);
            std::vector<uint32_t> words(plan.plain);
            words.insert(words.end(), plan.folded.begin(), plan.folded.end());
            words.insert(words.end(), plan.bypass.begin(), plan.bypass.end());
            s->leafOneToOne = true;
            for (const std::vector<uint32_t>* links : { &plan.plain, &plan.folded, &plan.bypass }) {
                const wptw::LeafWords leaf = wptw::leafWords(links->data(), desc->node_count, desc->tri_count);
                if (leaf.verdict == wptw::TOO_LARGE)
                    return fail(WPT_ERR_UNSUPPORTED, "a tree that fits LDS has indices beyond its leaf words");
                s->leafOneToOne = s->leafOneToOne && leaf.verdict == wptw::ONE_TO_ONE;
                words.insert(words.end(), leaf.words.begin(), leaf.words.end());
            }
            const uint32_t* onDevice = nullptr;
            WPT_TRY(uploadArray(s, words.data(), words.size(), &onDevice));
            s->ldsLinks = const_cast<uint32_t*>(onDevice);
            s->bypassedNodes = plan.outCount;
        }
    }
    {
        const std::vector<wpt_tri_attr> a = wptl::permuted(desc->tri_attr, triNew);
        WPT_TRY(uploadArray(s, reinterpret_cast<const float4*>(a.data()), size_t(desc->tri_count) * 6, &view.triAttr));
    }
    WPT_TRY(uploadArray(s, desc->instances, desc->instance_count, &view.instances));
    WPT_TRY(uploadArray(s, desc->materials, desc->material_count, &view.materials));
    view.materialCount = desc->material_count;
    {
        size_t texelCount = 0;
        const std::vector<wpt_texture> devTex = wptl::texelOffsets(desc, &texelCount);
        WPT_TRY(uploadArray(s, devTex.data(), devTex.size(), &view.textures));
        WPT_TRY(decodeTexels(s, desc, devTex, texelCount));
    }
    {
        const std::vector<wpt_hotspot> h = wptl::remappedHotspots(desc, triNew);
        WPT_TRY(uploadArray(s, h.data(), h.size(), &view.hotspots));
    }
    WPT_TRY(uploadArray(s, desc->spheres, desc->sphere_count, &view.spheres));
    WPT_TRY(uploadArray(s, desc->rgl_brdfs, desc->rgl_count, &view.rglBrdfs));
    {
        const wptl::RglPool rgl = wptl::rglPool(desc);
        WPT_TRY(uploadArray(s, rgl.pool.data(), rgl.pool.size(), &view.rglData));
        WPT_TRY(uploadArray(s, rgl.rgbl.data(), rgl.rgbl.size(), &view.rglRgbl));
    }
    WPT_TRY(uploadArray(s, desc->animations, desc->animation_count, &view.animations));
    WPT_TRY(uploadArray(s, desc->keyframes, desc->keyframe_count, &view.keyframes));
    s->animationCount = desc->animation_count;
    view.sphereCount = desc->sphere_count;
    for (int k = 0; k < 6; k++)
        view.envCube[k] = desc->envmap.cube_tex[k];
    {
        hipDeviceProp_t prop;
        s->cuCount = hipGetDeviceProperties(&prop, s->device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    view.triCount = desc->tri_count;
    view.hotspotCount = desc->hotspot_count;
    view.invHotspotCount = desc->hotspot_count ? 1.0f / float(desc->hotspot_count) : 0.0f;
    if (desc->hotspot_count > 0)
        WPT_TRY(hotspotFaces(s));
    view.envType = desc->envmap.type;
    view.envCompat = desc->envmap.compat;
    view.envTex = desc->envmap.tex;
    view.envN = 0;
    view.envLog2N = -1;
    if (desc->envmap.type != WPT_ENV_NONE && desc->envmap.N > 0) {
        const int N = desc->envmap.N;
        const size_t bins = size_t(N) * N;
        if (desc->envmap.M && desc->envmap.Ms && desc->envmap.Mcs) {
            s->envM.assign(desc->envmap.M, desc->envmap.M + bins);
            s->envMs.assign(desc->envmap.Ms, desc->envmap.Ms + bins);
            s->envMcs.assign(desc->envmap.Mcs, desc->envmap.Mcs + bins);
        } else {
            /* the per-bin importance comes from the device's own L(); the tables from it on the host */
            std::vector<float> importance;
            WPT_TRY(envImportance(view, N, &importance));
            wptl::EnvTables t = wptl::envTablesFromImportance(importance.data(), bins);
            s->envM.swap(t.M);
            s->envMs.swap(t.Ms);
            s->envMcs.swap(t.Mcs);
        }
        WPT_TRY(uploadArray(s, s->envM.data(), bins, &view.envM));
        WPT_TRY(uploadArray(s, s->envMs.data(), bins, &view.envMs));
        WPT_TRY(uploadArray(s, s->envMcs.data(), bins, &view.envMcs));
        const std::vector<int32_t> lut = wptl::envStartTable(s->envMcs.data(), bins);
        if (!lut.empty()) { /* a caller's own table that is not monotone gets the plain bisection */
            WPT_TRY(uploadArray(s, lut.data(), lut.size(), &view.envLut));
            view.envLutSize = wptl::ENV_LUT_SIZE;
        }
        view.envN = N;
        view.envLog2N = wptl::envLog2(N);
    }
    *out_scene = owner.release();
    return WPT_OK;
}

void wpt_scene_free(wpt_scene* scene)
{
    if (!scene)
        return;
    for (void* p : scene->allocations)
        (void)hipFree(p);
    delete scene;
}

/* copies the importance tables of an uploaded scene back (tests compare them with the oracle's) */
wpt_status wpt_scene_get_envmap_tables(const wpt_scene* scene, float* M, int32_t* Ms, float* Mcs)
{
    if (!scene || scene->view.envN <= 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "scene has no importance tables");
    size_t bins = scene->envM.size();
    memcpy(M, scene->envM.data(), bins * sizeof(float));
    memcpy(Ms, scene->envMs.data(), bins * sizeof(int32_t));
    memcpy(Mcs, scene->envMcs.data(), bins * sizeof(float));
    return WPT_OK;
}

} /* extern "C" */

namespace {

/* The frame and block checks of every render call, one text each.  samplesSqrt: NULL where the call has none (an adaptive map
 * holds the counts); the block must lie in `frames` frames of width * height pixels (a batch of views: one per camera); prefix:
 * what the entry point's messages begin with; session: an empty block is refused too. */
wpt_status checkFrameBlock(uint32_t width, uint32_t height, const uint32_t* samplesSqrt, uint32_t blockStart, uint32_t blockSize,
        uint32_t frames = 1, const char* prefix = "", bool session = false)
{
    if (width == 0 || height == 0 || width > 65535 || height > 65535 || (samplesSqrt && (*samplesSqrt == 0 || *samplesSqrt > 65535)))
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(prefix) + (samplesSqrt ? "width, height and samples_sqrt" : "width and height")
                + " must lie in 1 .. 65535");
    /* (width * height fits 32 bits after the check above) */
    if ((session && blockSize == 0) || uint64_t(blockStart) + blockSize > uint64_t(width) * height * frames)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(prefix) + (session ? "pixel block is empty or lies outside the frame"
                : "pixel block lies outside the frame"));
    return WPT_OK;
}

/* What every launch of the single kernel sets up the same way, a plain block, bands, a batch of views or a stage of a session
 * (wpt_progress_begin): the frame's constants, the 8x8 tiles, the features the cameras add to the scene's, the scheduler's
 * settings.  `camera` is the first of cameraCount cameras (batch: they are a batch of views); frame, counters, the sensor's
 * view and what a stage adds are the caller's. */
wpt_status launchSetUp(const wpt_scene* scene, const wpt_camera* camera, uint32_t cameraCount, bool batch, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        uint32_t band_pixels, uint32_t band_first, uint32_t band_stride, bool count, wptk::KernelArgs& args, uint32_t& need)
{
    args.bandPixels = band_pixels;
    args.bandFirst = band_first;
    args.bandStride = band_stride;
    args.sv = scene->view;
    args.cam = *camera;
    args.par = *params;
    args.width = width;
    args.height = height;
    args.samplesSqrt = samples_sqrt;
    args.invWidth = 1.0f / float(width);
    args.invHeight = 1.0f / float(height);
    args.invSamplesSqrt = 1.0f / float(samples_sqrt);
    args.invSamples = 1.0f / float(samples_sqrt * samples_sqrt);
    args.blockStart = block_start;
    args.blockSize = block_size;
    args.fuse = (g_variant & 0x20u) ? 0u : 1u; /* variant bit 0x20: separate SHADE / NEE-END / NEW rounds (the older scheduler) */

    /* a wave covers an 8x8 pixel tile when the block consists of whole groups of 8 rows */
    args.tiled = (width % 8 == 0 && block_start % width == 0 && block_size % (8 * width) == 0
            && (band_stride == 0 || band_pixels % (8 * width) == 0)) ? 1u : 0u;
    if (batch) /* 8x8 tiles within each view's frame */
        args.tiled = (width % 8 == 0 && height % 8 == 0) ? 1u : 0u;
    /* a batch takes the union of the scene's features and every camera's */
    need = scene->features;
    for (uint32_t v = 0; v < cameraCount; v++) {
        const wpt_camera* c = camera + v;
        need |= (c->lens_radius > 0.0f || c->distortion_type != WPT_DISTORTION_NONE || c->surround_mode != WPT_SURROUND_OFF
                || c->stereoscopic_distance > 0.0f) ? FEAT_LENS : 0u;
        if (c->surround_mode > WPT_SURROUND_360)
            return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
        if (c->distortion_type > WPT_DISTORTION_OPENCV)
            return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
        if (c->animation >= int32_t(scene->animationCount))
            return fail(WPT_ERR_INVALID_ARGUMENT, batch ? "camera " + std::to_string(v) + " refers to an animation outside the scene's array"
                    : std::string("camera refers to an animation outside the scene's array"));
        if (batch && c->animation >= 0) /* an animated camera selects the moving-scene kernels */
            need |= FEAT_ANIM;
    }
    /* an exposure interval changes every path (each camera ray draws its time), moving instances need the time too */
    if (params->t0 != params->t1)
        need |= FEAT_ANIM;
    /* The walk of a light ray towards the environment ends at its first accepted hit (wpt_pathtrace.inc.h: the answer it is
     * traced for is known there).  Counting launches walk on as the reference does, so that their counters are the
     * reference's; measurements (wpt_set_walk): WPT_WALK_COUNT_PRODUCT makes them count what the product kernel walks,
     * WPT_WALK_FULL_SHADOW switches the short cut off everywhere. */
    args.shadowWalksEnd = (g_walk & WPT_WALK_FULL_SHADOW) ? 0u : (count ? ((g_walk & WPT_WALK_COUNT_PRODUCT) ? 1u : 0u) : 1u);
    /* scheduler defaults from sweeps on the Cornell box (scene in LDS, short walks) and on the
     * Sponza-class scene (deep tree in HBM: traversal dominates, so long blocks may run with fewer
     * lanes and leaf tests earlier) */
    const bool smallScene = size_t(scene->nodeCount) * 32 + size_t(scene->triCount) * 48 <= LDS_SCENE_MAX_BYTES;
    /* clamped: with more than 8 eighths the traversal block would leave before doing anything */
    args.leaveEighths = g_leaveEighths ? (g_leaveEighths > 8u ? 8u : g_leaveEighths) : (smallScene ? 1u : 3u);
    args.heavyMin = g_heavyMin ? g_heavyMin : (smallScene ? 16u : 8u);
    args.leafBias = g_leafBias ? g_leafBias : (smallScene ? 16u : 32u);
    /* variant bits 2-3: 0 = default, 1 = no kind of material ever stands back, 2 / 3 = fewer than 3 / 12 lanes */
    static const uint32_t waitBelowChoices[4] = { 6u, 0u, 3u, 12u };
    args.waitBelow = waitBelowChoices[(g_variant >> 2) & 0x3u];
    args.cuCount = uint32_t(scene->cuCount);
    return WPT_OK;
}

/* One launch of the path tracer: a block of consecutive pixels (bandStride == 0) or interleaved bands of bandPixels pixels, and
 * the one sensor it renders for, whose view is the member that `sensor` names.  Every caller sets the first ten members. */
struct LaunchRequest {
    wpt_scene* scene;
    const wpt_camera* camera; /* SENSOR_VIEWS: the first of views.viewCount host cameras, the block all their pixels */
    const wpt_params* params;
    uint32_t width, height, samplesSqrt, blockStart, blockSize;
    float* frame; /* may be NULL for the transient film and for several time-of-flight phases */
    void* stream;
    wpt_counters* counters = nullptr;
    uint32_t bandPixels = 0, bandFirst = 0, bandStride = 0;
    wptk::Sensor sensor = wptk::SENSOR_FRAME;
    wptk::BinsView bins = {};         /* SENSOR_TRANSIENT, SENSOR_TOF (wpt_blocks.h, accumulate) */
    wptk::ViewsView views = {};       /* SENSOR_VIEWS */
    wptk::AdaptiveView adaptive = {}; /* SENSOR_ADAPTIVE */
};

/* The stream-ordered scratch memory of one launch (the pool's counter, carry, cost, order, work words, slice words and carry):
 * launches in flight on any number of streams never share any of it; freed in stream order when the owner goes out of scope,
 * behind the read of the launch's error. */
struct StreamScratch {
    hipStream_t stream;
    void* held[5] = {}; /* the counter and the four arrays of two passes: no launch asks for more */
    uint32_t count = 0;
    explicit StreamScratch(hipStream_t s) : stream(s) {}
    StreamScratch(const StreamScratch&) = delete;
    ~StreamScratch()
    {
        for (uint32_t i = 0; i < count; i++)
            (void)hipFreeAsync(held[i], stream);
    }
    /* n elements, or NULL where the memory cannot be had: the error is cleared, the launch goes without */
    template<typename T> T* get(size_t n)
    {
        void* p = nullptr;
        assert(count < sizeof(held) / sizeof(held[0]));
        if (hipMallocAsync(&p, n * sizeof(T), stream) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return static_cast<T*>(held[count++] = p);
    }
};

/* the single kernel of a launch, as every execution below launches it */
struct SingleKernel {
    const wptk::KernelEntry* kernel;
    dim3 grid;
    size_t sceneLdsBytes;
    hipStream_t stream;
    void operator()(const wptk::KernelArgs& a) const { kernel->launch(a, grid, sceneLdsBytes, stream); }
};

/* the work words of the order kernels (wpt_k_order.hip); the last is the number of entries of the order they build */
constexpr size_t ORDER_WORK_WORDS = 3 * wptk::ORDER_BUCKETS + 1;

/* `order` from the costs `measured` left per pixel, the costliest 8x8 tiles first, for `next` to take its pixels in */
void orderByCost(const wptk::KernelArgs& measured, uint32_t* order, uint32_t* work, hipStream_t stream, wptk::KernelArgs& next)
{
    wptk::launchOrderBuild(measured, order, work, stream);
    next.order = order;
    next.orderCount = work + ORDER_WORK_WORDS - 1;
}

/* TWO_PASSES: one timed row of strata of every pixel, then the rest in the order of those times.  false, and nothing
 * launched: the memory cannot be had. */
bool runTwoPasses(const wptk::KernelArgs& args, const SingleKernel& run, StreamScratch& scratch)
{
    const size_t pixels = size_t(args.width) * args.height;
    float4* carry;
    uint32_t *cost, *order, *work;
    if (!(carry = scratch.get<float4>(pixels * 2)) || !(cost = scratch.get<uint32_t>(pixels)) || !(order = scratch.get<uint32_t>(args.blockSize))
            || !(work = scratch.get<uint32_t>(ORDER_WORK_WORDS)))
        return false;
    wptk::KernelArgs first = args, second = args;
    first.rowStop = 1;
    first.carry = second.carry = carry;
    first.cost = cost;
    run(first);
    orderByCost(first, order, work, run.stream, second);
    run(second);
    return true;
}

/* ADAPTIVE_ORDER: one pass in the order built from the sample counts n^2 of the map.  false as above. */
bool runAdaptiveOrder(const wptk::KernelArgs& args, const SingleKernel& run, StreamScratch& scratch)
{
    uint32_t *cost, *order, *work;
    if (!(cost = scratch.get<uint32_t>(args.blockSize)) || !(order = scratch.get<uint32_t>(args.blockSize)) || !(work = scratch.get<uint32_t>(ORDER_WORK_WORDS)))
        return false;
    wptk::KernelArgs measure = args, ordered = args;
    measure.cost = cost - args.blockStart; /* indexed by the frame's pixel: the block's pixels land in the allocation */
    wptk::launchAdaptiveCost(measure, run.stream);
    orderByCost(measure, order, work, run.stream, ordered);
    run(ordered);
    return true;
}

/* SLICED: one launch of the kernel's twin that hands the pixels out in plan.units units of plan.rows rows.  Returns the
 * counters the launch adds to (wpt_last_slice_stats), or NULL and nothing launched: they or the memory cannot be had. */
unsigned long long* runSliced(const wptk::KernelArgs& args, const SingleKernel& runTwin, const wptk::LaunchPlan& plan, StreamScratch& scratch)
{
    unsigned long long* stats = sliceStatsOfCurrentDevice();
    float4* carry;
    uint32_t* words;
    if (!stats || !(carry = scratch.get<float4>(size_t(args.blockSize) * 2)) || !(words = scratch.get<uint32_t>(args.blockSize)))
        return nullptr;
    if (hipMemsetAsync(words, 0, size_t(args.blockSize) * sizeof(uint32_t), runTwin.stream) != hipSuccess
            || hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), runTwin.stream) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    wptk::KernelArgs inSlices = args;
    inSlices.slices = { words, carry, stats, plan.rows, plan.units, (g_slices & WPT_SLICES_DECLINE_ODD) ? 1u : 0u };
    runTwin(inSlices);
    return stats;
}

/* The single kernel by the plan's strategy, and the pool's counter where the plan has one.  Where the memory a strategy needs
 * cannot be had (the counter first of all), one plain pass renders the launch.  Returns the launch's error. */
hipError_t runSingleKernel(const wpt_scene* scene, wptk::KernelArgs& args, const wptk::KernelChoice& choice, const wptk::KernelEntry* kernel,
        const wptk::KernelEntry* slicedTwin, const wptk::LaunchPlan& plan, hipStream_t stream)
{
    StreamScratch scratch(stream);
    args.pool = plan.pooled ? scratch.get<uint32_t>(1) : nullptr;
    args.materialsInLds = choice.materialsInLds;
    if (choice.ldsScene) {
        /* The link words of the tree's copy in LDS.  Exact: the fold's, or every node's own under WPT_WALK_NO_FOLD; the launch's:
         * the ones that go round the nodes the scene's plan leaves out -- they are built on the fold, so not under NO_FOLD, not
         * under WPT_WALK_NO_BYPASS, and not for a tree with a NaN bound, whose rays all keep the exact links. */
        if (!scene->ldsLinks)
            return hipErrorInvalidValue; /* (every scene that fits LDS has them) */
        const size_t words = 2 * size_t(scene->nodeCount) + 4;
        const bool fold = (choice.materialsInLds & wptk::LDS_FOLD) != 0;
        const bool bypass = fold && !(g_walk & WPT_WALK_NO_BYPASS) && !args.sv.boxesMayBeNan;
        args.sv.spheres = reinterpret_cast<const wpt_sphere*>(scene->ldsLinks + (fold ? words : 0));
        args.sv.wideNodes = reinterpret_cast<const float4*>(scene->ldsLinks + (bypass ? 2 * words : fold ? words : 0));
        if (choice.rotated) {
            /* the same sets with the leaf words of the rotated kernels (wpt_leaf_words.h) */
            const size_t leafWords = wptw::leafWordsSize(scene->nodeCount, scene->triCount);
            const uint32_t* sets = scene->ldsLinks + 3 * words;
            args.sv.spheres = reinterpret_cast<const wpt_sphere*>(sets + (fold ? leafWords : 0));
            args.sv.wideNodes = reinterpret_cast<const float4*>(sets + (bypass ? 2 * leafWords : fold ? leafWords : 0));
            if (scene->leafOneToOne)
                args.materialsInLds |= wptk::LDS_LEAF_LINKS;
        }
    }
    const SingleKernel run = { kernel, dim3((args.blockSize + WG - 1) / WG), choice.sceneLdsBytes, stream };
    bool done = false;
    unsigned long long* sliceStats = nullptr;
    if (args.pool && plan.strategy == wptk::TWO_PASSES)
        done = runTwoPasses(args, run, scratch);
    else if (args.pool && plan.strategy == wptk::ADAPTIVE_ORDER)
        done = runAdaptiveOrder(args, run, scratch);
    else if (args.pool && plan.strategy == wptk::SLICED)
        done = (sliceStats = runSliced(args, SingleKernel{ slicedTwin, run.grid, run.sceneLdsBytes, stream }, plan, scratch)) != nullptr;
    if (!done)
        run(args);
    recordLaunch(kernel->name, kernelForm(choice.rotated, sliceStats ? plan.units : 0, choice.rotated && !scene->leafOneToOne), done ? plan.passes : 1u,
            sliceStats);
    return hipGetLastError();
}

/* one launch, in five steps: check, set up, choose the kernel (wpt_kernel_table.h), plan its passes (wpt_launch_plan.h), execute */
wpt_status renderLaunch(const LaunchRequest& rq)
{
    const bool planes = rq.sensor == wptk::SENSOR_TRANSIENT || rq.sensor == wptk::SENSOR_TOF, views = rq.sensor == wptk::SENSOR_VIEWS;
    if (!rq.scene || !rq.camera || !rq.params || !(rq.frame || planes))
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const uint32_t cameraCount = views ? rq.views.viewCount : 1u;
    const wpt_status checked = checkFrameBlock(rq.width, rq.height, &rq.samplesSqrt, rq.blockStart, rq.bandStride ? 0u : rq.blockSize, cameraCount);
    if (checked != WPT_OK || rq.blockSize == 0)
        return checked;
    KernelArgs args = {};
    uint32_t need = 0;
    const bool count = rq.counters != nullptr;
    WPT_TRY(launchSetUp(rq.scene, rq.camera, cameraCount, views, rq.params, rq.width, rq.height, rq.samplesSqrt, rq.blockStart,
            rq.blockSize, rq.bandPixels, rq.bandFirst, rq.bandStride, count, args, need));
    args.frame = rq.frame;
    args.counters = rq.counters;
    args.schedStats = g_schedStats;
    if (views)
        args.views = rq.views;
    else if (rq.sensor == wptk::SENSOR_ADAPTIVE)
        args.adaptive = rq.adaptive;
    else if (planes)
        args.bins = rq.bins;
    args.rowStop = rq.samplesSqrt;
    const wptk::KernelChoice choice = wptk::selectKernel({ need, rq.sensor, count, rq.scene->nodeCount, rq.scene->triCount,
            uint32_t(rq.scene->view.materialCount), rq.scene->view.wideNodes != nullptr, g_variant, g_walk });
    const wptk::KernelEntry *kernel = nullptr, *slicedTwin = nullptr;
    wpt_status found = lookupKernel(choice.features, choice.count, choice.ldsScene, choice.wide, &kernel);
    /* its twin that hands pixels out in slices, for a SLICED plan */
    if (found == WPT_OK && choice.sceneInLds && rq.sensor == wptk::SENSOR_FRAME && !count)
        found = lookupKernel(choice.features | FEAT_SLICED, choice.count, choice.ldsScene, choice.wide, &slicedTwin);
    if (found != WPT_OK)
        return found;
    const bool rgl = (need & FEAT_RGL) != 0;
    hipStream_t stream = static_cast<hipStream_t>(rq.stream);
    const wptk::LaunchPlan plan = wptk::planLaunch({ rq.sensor, count, rgl, (need & FEAT_ANIM) != 0, choice.sceneInLds, rq.blockSize, rq.samplesSqrt,
            uint32_t(rq.scene->cuCount), g_variant, g_wfMode, g_slices });
    if (plan.wavefront) {
        uint32_t launches = 0; /* of trace and shade, two kernels that hand rays through HBM (wpt_wavefront.inc.h) */
        const hipError_t e = wptk::renderWavefront(args, rgl ? wptk::wfFullRgl() : (choice.basic ? wptk::wfBasic() : wptk::wfFull()), g_wfConfig, stream, &launches);
        if (e == hipSuccess) {
            recordLaunch("wf_trace + wf_shade", "", launches, nullptr);
            return WPT_OK;
        }
        /* the library's own choice must not fail where the single kernel would not: without the memory for the records (256 B
         * per lane) that one renders the frame; a forced wavefront render reports the error */
        if (!plan.wavefrontFallBack || e != hipErrorOutOfMemory)
            return fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("wavefront render: ") + hipGetErrorString(e));
        (void)hipGetLastError();
    }
    HIP_TRY(runSingleKernel(rq.scene, args, choice, kernel, slicedTwin, plan, stream));
    return WPT_OK;
}

/* Device memory of a host entry point for a block's pixels only, not a frame's: the launch gets a pointer biased so that pixel
 * `blockStart` lands at offset 0.  Freed at scope exit. */
struct StagedBlock {
    void* device = nullptr;
    size_t bytes = 0;
    StagedBlock() = default;
    StagedBlock(const StagedBlock&) = delete;
    ~StagedBlock() { (void)hipFree(device); }
    hipError_t allocate(size_t n) { return hipMalloc(&device, bytes = n); }
    hipError_t allocatePixels(size_t pixels, size_t planes = 1) { return allocate(pixels * 3 * sizeof(float) * planes); }
    hipError_t upload(const void* host) { return hipMemcpy(device, host, bytes, hipMemcpyHostToDevice); }
    hipError_t download(void* host) const { return device ? hipMemcpy(host, device, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    /* NULL without memory: an output the caller did not ask for */
    float* biased(uint32_t blockStart) const { return device ? static_cast<float*>(device) - size_t(blockStart) * 3 : nullptr; }
};

/* The end of a host entry point: behind a launch that went well, waits for the device and reports what its kernels ran into
 * (wpt_scene_check; check == NULL: the launch is not the scene's), then copies the staged blocks that exist to their host arrays. */
wpt_status finishStaged(wpt_status launched, wpt_scene* check, const StagedBlock& a, void* hostA, const StagedBlock* b = nullptr, void* hostB = nullptr)
{
    const wpt_status st = launched == WPT_OK && check ? wpt_scene_check(check) : launched;
    hipError_t e = st == WPT_OK ? a.download(hostA) : hipSuccess;
    if (st == WPT_OK && e == hipSuccess && b)
        e = b->download(hostB);
    return e == hipSuccess ? st : fail(WPT_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
}

} /* namespace */

extern "C" {

wpt_status wpt_render_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame_device, hip_stream };
    rq.counters = counters_device;
    return renderLaunch(rq);
}

wpt_status wpt_render_bands_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream)
{
    if (band_rows == 0 || band_stride == 0 || first_band >= band_stride || width == 0 || height == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands need band_rows > 0 and first_band < band_stride");
    const uint64_t bandPixels = uint64_t(band_rows) * width;
    const uint64_t bands = (uint64_t(height) + band_rows - 1) / band_rows;
    const uint64_t mine = first_band < bands ? (bands - first_band + band_stride - 1) / band_stride : 0;
    if (bandPixels > 0xffffffffull || mine * bandPixels > 0xffffffffull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands too large");
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, 0, uint32_t(mine * bandPixels), frame_device, hip_stream };
    rq.bandPixels = uint32_t(bandPixels);
    rq.bandFirst = first_band;
    rq.bandStride = band_stride;
    rq.counters = counters_device;
    return renderLaunch(rq);
}

wpt_status wpt_render_bands(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host)
{
    if (!frame_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "frame_host is NULL");
    if (width == 0 || height == 0 || band_rows == 0 || band_stride == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bands need a frame, band_rows > 0 and band_stride > 0");
    float* dFrame = nullptr;
    const size_t rowBytes = size_t(width) * 3 * sizeof(float);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dFrame), rowBytes * height));
    wpt_status st = wpt_render_bands_device(scene, camera, params, width, height, samples_sqrt, band_rows, first_band, band_stride, dFrame, nullptr,
            nullptr);
    if (st == WPT_OK)
        st = wpt_scene_check(scene);
    for (uint64_t band = first_band; st == WPT_OK && band * band_rows < height; band += band_stride) {
        const size_t row0 = size_t(band) * band_rows;
        const size_t rows = row0 + band_rows <= height ? band_rows : height - row0;
        hipError_t e = hipMemcpy(reinterpret_cast<char*>(frame_host) + row0 * rowBytes, reinterpret_cast<char*>(dFrame) + row0 * rowBytes, rows * rowBytes,
                hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    (void)hipFree(dFrame);
    return st;
}

wpt_status wpt_render_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width,
        uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb)
{
    if (!block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_rgb is NULL");
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block;
    HIP_TRY(block.allocatePixels(block_size));
    return finishStaged(wpt_render_block_device(scene, camera, params, width, height, samples_sqrt, block_start, block_size,
            block.biased(block_start), nullptr, nullptr), scene, block, block_rgb);
}

} /* extern "C" */

/* ---- a frame in resumable stages (wurblpt_hip.h: progressive sessions) ---- */

struct wpt_progress {
    wpt_scene* scene;
    wptk::KernelArgs args; /* of the one-shot launch of the block; a stage sets frame, rowStop, order, orderCount and pool */
    wptk::KernelChoice choice;
    const wptk::KernelEntry* kernel;
    uint32_t rowsDone;
    uint64_t tag;
    /* device memory for the session's lifetime: carry and cost per pixel of the frame (the kernels index them by the frame's
     * pixel), order per pixel of the block, the order kernels' work words */
    float4* carry;
    uint32_t *cost, *order, *work;
    bool frameOrderBuilt; /* scene in LDS: `order` holds the frame's own order, which every later stage takes */
    hipStream_t lastStream;
};

namespace {

void progressFree(wpt_progress* p)
{
    for (void* m : { static_cast<void*>(p->carry), static_cast<void*>(p->cost), static_cast<void*>(p->order), static_cast<void*>(p->work) })
        if (m)
            (void)hipFree(m);
    delete p;
}

wpt_progress_info progressInfo(const wpt_progress* p)
{
    wpt_progress_info i;
    memset(&i, 0, sizeof(i));
    i.version = WPT_PROGRESS_STATE_VERSION;
    i.width = p->args.width;
    i.height = p->args.height;
    i.samples_sqrt = p->args.samplesSqrt;
    i.block_start = p->args.blockStart;
    i.block_size = p->args.blockSize;
    i.rows_done = p->rowsDone;
    i.tag = p->tag;
    i.state_bytes = uint64_t(wptp::STATE_HEADER_BYTES) + uint64_t(i.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL;
    return i;
}

}

extern "C" {

wpt_status wpt_progress_covers(uint32_t sensor, uint32_t counting, uint32_t bands)
{
    static const char* const sensors[] = { nullptr, "the transient film", "a batch of views", "an adaptive map", "the time-of-flight sensor" };
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor must lie in 0 .. 4");
    if (sensors[sensor])
        return fail(WPT_ERR_UNSUPPORTED, std::string("sessions render one frame, not ") + sensors[sensor]
                + ": what a pixel carries between stages is its generator and three sums");
    if (counting)
        return fail(WPT_ERR_UNSUPPORTED, "sessions do not cover counting launches: the counters of a stage would count the launch's lanes, not the rows rendered");
    if (bands)
        return fail(WPT_ERR_UNSUPPORTED, "sessions do not cover bands: a session renders one block of consecutive pixels");
    return WPT_OK;
}

wpt_status wpt_progress_begin(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, uint64_t tag, wpt_progress** out_progress)
{
    if (out_progress)
        *out_progress = nullptr;
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; the path tracer has no CPU fallback");
    if (!scene || !camera || !params || !out_progress)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(checkFrameBlock(width, height, &samples_sqrt, block_start, block_size, 1, "", true));
    /* the arguments and the kernel of the plain frame launch without counters, set up by what renderLaunch sets them up with */
    wpt_progress* p = new wpt_progress{}; /* (zeros: no row done, no memory yet, the null stream) */
    p->scene = scene;
    p->tag = tag;
    KernelArgs& args = p->args;
    uint32_t need = 0;
    const wpt_status setUp = launchSetUp(scene, camera, 1, false, params, width, height, samples_sqrt, block_start, block_size, 0, 0, 0, false, args, need);
    if (setUp != WPT_OK) {
        progressFree(p);
        return setUp;
    }
    args.bins = wptk::BinsView{};
    p->choice = wptk::selectKernel({ need, wptk::SENSOR_FRAME, false, scene->nodeCount, scene->triCount, uint32_t(scene->view.materialCount),
            scene->view.wideNodes != nullptr, g_variant, g_walk });
    const wpt_status found = lookupKernel(p->choice.features, p->choice.count, p->choice.ldsScene, p->choice.wide, &p->kernel);
    if (found != WPT_OK) {
        progressFree(p);
        return found;
    }
    args.materialsInLds = p->choice.materialsInLds;
    /* hipMalloc, not stream-ordered: the memory outlives the calls.  Carry and cost start as zeros: a state saved before the
     * first stage is defined, and so is the order that a restored session builds from times it never measured. */
    const size_t pixels = size_t(width) * height;
    const size_t workBytes = ORDER_WORK_WORDS * sizeof(uint32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->carry), pixels * 2 * sizeof(float4));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->cost), pixels * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->order), size_t(block_size) * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&p->work), workBytes);
    if (e == hipSuccess)
        e = hipMemset(p->carry + 2 * size_t(block_start), 0, size_t(block_size) * 2 * sizeof(float4));
    if (e == hipSuccess)
        e = hipMemset(p->cost, 0, pixels * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        progressFree(p);
        return fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("session memory (40 bytes per pixel): ") + hipGetErrorString(e));
    }
    args.carry = p->carry;
    args.cost = p->cost;
    *out_progress = p;
    return WPT_OK;
}

wpt_status wpt_progress_advance_device(wpt_progress* p, uint32_t rows, float* frame_device, void* hip_stream)
{
    if (!p)
        return fail(WPT_ERR_INVALID_ARGUMENT, "progress is NULL");
    const uint32_t total = p->args.samplesSqrt;
    if (rows == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "a stage renders at least one row of strata: rows is 0");
    if (p->rowsDone >= total)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the session is finished: all " + std::to_string(total) + " rows of strata are rendered");
    const uint32_t rowStop = rows < total - p->rowsDone ? p->rowsDone + rows : total;
    if (rowStop == total && !frame_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the stage that finishes the frame needs frame_device: it is NULL");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    wptk::KernelArgs stage = p->args;
    stage.frame = frame_device;
    stage.rowStop = rowStop;
    stage.schedStats = nullptr;
    if (p->rowsDone > 0 && !p->choice.sceneInLds) {
        /* a stage that resumes takes its pixels from `order` and loads what they carry: for the scene in HBM the tiles that
         * took the stage before longest first, as the second of the one-shot launch's two passes does */
        orderByCost(p->args, p->order, p->work, stream, stage);
    } else if (p->rowsDone > 0) {
        /* ... and the frame's own order for the scene in LDS (any other costs those kernels more than it gains) */
        if (!p->frameOrderBuilt)
            wptk::launchProgressFrameOrder(p->args, p->order, p->work + ORDER_WORK_WORDS - 1, stream);
        p->frameOrderBuilt = true;
        stage.order = p->order;
        stage.orderCount = p->work + ORDER_WORK_WORDS - 1;
    }
    /* planned as a frame launch without counters (with the variant word of this moment) whose strategy the session has fixed:
     * one pass, in the order set up above */
    const bool pooled = wptk::planLaunch({ wptk::SENSOR_FRAME, false, false, false, p->choice.sceneInLds, stage.blockSize, total, stage.cuCount,
            g_variant, 2u, 1u }).pooled;
    HIP_TRY(runSingleKernel(p->scene, stage, p->choice, p->kernel, nullptr, { false, false, pooled, wptk::ONE_PASS, 1, total, 1 }, stream));
    /* The launch that renders the last row writes the frame and stores no carry.  A finished session keeps the block's pixels
     * of its frame in the carry's place instead, so that its preview and its saved state still yield the frame. */
    if (rowStop == total) {
        wptk::launchProgressCapture(frame_device, p->carry, p->args.blockStart, p->args.blockSize, total << 16, stream);
        HIP_TRY(hipGetLastError());
    }
    p->rowsDone = rowStop;
    p->lastStream = stream;
    return WPT_OK;
}

wpt_status wpt_progress_advance(wpt_progress* p, uint32_t rows, float* block_rgb)
{
    if (!p)
        return fail(WPT_ERR_INVALID_ARGUMENT, "progress is NULL");
    const uint32_t total = p->args.samplesSqrt;
    const bool finishes = rows > 0 && p->rowsDone < total && rows >= total - p->rowsDone;
    if (finishes && !block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the stage that finishes the frame needs block_rgb: it is NULL");
    StagedBlock block;
    if (finishes)
        HIP_TRY(block.allocatePixels(p->args.blockSize));
    return finishStaged(wpt_progress_advance_device(p, rows, block.biased(p->args.blockStart), nullptr), p->scene, block, block_rgb);
}

uint32_t wpt_progress_rows_done(const wpt_progress* p)
{
    return p ? p->rowsDone : 0u;
}

uint32_t wpt_progress_rows_total(const wpt_progress* p)
{
    return p ? p->args.samplesSqrt : 0u;
}

wpt_status wpt_progress_preview_device(wpt_progress* p, float* frame_device, void* hip_stream)
{
    if (!p || !frame_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* (a finished session's carry holds the pixels' values themselves, and a session without a stage zeros) */
    const uint32_t total = p->args.samplesSqrt;
    const float inv = p->rowsDone == total ? 1.0f : (p->rowsDone ? 1.0f / float(p->rowsDone * total) : 0.0f);
    wptk::launchProgressResolve(p->carry, frame_device, p->args.blockStart, p->args.blockSize, inv, stream);
    HIP_TRY(hipGetLastError());
    p->lastStream = stream;
    return WPT_OK;
}

wpt_status wpt_progress_preview(wpt_progress* p, float* block_rgb)
{
    if (!p || !block_rgb)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock block;
    HIP_TRY(hipStreamSynchronize(p->lastStream));
    HIP_TRY(block.allocatePixels(p->args.blockSize));
    return finishStaged(wpt_progress_preview_device(p, block.biased(p->args.blockStart), nullptr), nullptr, block, block_rgb);
}

void wpt_progress_end(wpt_progress* p)
{
    if (!p)
        return;
    (void)hipStreamSynchronize(p->lastStream);
    progressFree(p);
}

wpt_status wpt_progress_state_bytes(const wpt_progress* p, uint64_t* bytes)
{
    if (!p || !bytes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *bytes = progressInfo(p).state_bytes;
    return WPT_OK;
}

wpt_status wpt_progress_save(wpt_progress* p, void* buffer_host, uint64_t bytes)
{
    if (!p || !buffer_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const wpt_progress_info info = progressInfo(p);
    if (bytes != info.state_bytes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the buffer must hold wpt_progress_state_bytes = " + std::to_string(info.state_bytes) + " bytes, not "
                + std::to_string(bytes));
    HIP_TRY(hipStreamSynchronize(p->lastStream));
    wptp::writeStateHeader(buffer_host, info, p->args.cam, p->args.par);
    HIP_TRY(hipMemcpy(static_cast<unsigned char*>(buffer_host) + wptp::STATE_HEADER_BYTES, p->carry + 2 * size_t(info.block_start),
            size_t(info.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL, hipMemcpyDeviceToHost));
    return WPT_OK;
}

wpt_status wpt_progress_state_info(const void* buffer_host, uint64_t bytes, wpt_progress_info* info)
{
    if (!info)
        return fail(WPT_ERR_INVALID_ARGUMENT, "info is NULL");
    if (bytes > uint64_t(SIZE_MAX))
        return fail(WPT_ERR_INVALID_ARGUMENT, "the state is longer than its header says");
    const char* refused = wptp::parseState(buffer_host, size_t(bytes), info);
    return refused ? fail(WPT_ERR_INVALID_ARGUMENT, refused) : WPT_OK;
}

wpt_status wpt_progress_restore(wpt_scene* scene, const void* buffer_host, uint64_t bytes, const wpt_camera* camera, const wpt_params* params,
        uint64_t tag, wpt_progress** out_progress)
{
    if (out_progress)
        *out_progress = nullptr;
    if (!scene || !camera || !params || !out_progress)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    wpt_progress_info info;
    const wpt_status parsed = wpt_progress_state_info(buffer_host, bytes, &info);
    if (parsed != WPT_OK)
        return parsed;
    const unsigned char* state = static_cast<const unsigned char*>(buffer_host);
    const char* differs = info.tag != tag ? "tag" : memcmp(state + wptp::STATE_CAMERA, camera, sizeof(*camera)) != 0 ? "camera"
            : memcmp(state + wptp::STATE_PARAMS, params, sizeof(*params)) != 0 ? "params" : nullptr;
    if (differs)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string("the state was saved with a different ") + differs);
    /* the body, as far as the header says what it holds: every pixel stands at the first stratum of row rows_done */
    const uint64_t damaged = wptp::firstDamagedRecord(state, info);
    if (damaged < info.block_size)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the state is damaged: the record of pixel " + std::to_string(uint64_t(info.block_start) + damaged)
                + " does not stand at row rows_done of its strata");
    wpt_progress* p = nullptr;
    const wpt_status begun = wpt_progress_begin(scene, camera, params, info.width, info.height, info.samples_sqrt, info.block_start, info.block_size,
            tag, &p);
    if (begun != WPT_OK)
        return begun;
    const hipError_t e = hipMemcpy(p->carry + 2 * size_t(info.block_start), state + wptp::STATE_HEADER_BYTES,
            size_t(info.block_size) * wptp::STATE_CARRY_BYTES_PER_PIXEL, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        progressFree(p);
        return fail(WPT_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    p->rowsDone = info.rows_done;
    *out_progress = p;
    return WPT_OK;
}

} /* extern "C" */

namespace {

/* the transient film's planes after the launch: plane value = 1 / samples * accumulated value (SensorRGB::finishPixel) for the
 * block's pixels of every plane */
__global__ void wpt_transient_finish_kernel(float* bins, size_t stride, uint32_t blockStart, uint32_t blockSize, uint32_t binCount, float invSamples)
{
    const uint64_t perPlane = uint64_t(blockSize) * 3, n = perPlane * binCount;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        float* p = bins + (i / perPlane) * stride + size_t(blockStart) * 3 + i % perPlane;
        *p = invSamples * *p;
    }
}

/* refuses a bad edge set; fills what the kernels need of a good one but the device copy of the edges */
wpt_status transientEdges(const float* edges, uint32_t binCount, wptk::BinsView& bv)
{
    if (!edges)
        return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edges are NULL");
    if (binCount == 0 || binCount > WPT_TRANSIENT_MAX_BINS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin count must lie in 1 .. " + std::to_string(WPT_TRANSIENT_MAX_BINS));
    for (uint32_t k = 0; k <= binCount; k++) {
        if (std::isnan(edges[k]))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edge " + std::to_string(k) + " is NaN");
        if (std::isinf(edges[k]) && !(k == binCount && edges[k] > 0.0f))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edge " + std::to_string(k) + " is infinite (only the last may be +inf)");
        if (k > 0 && !(edges[k] > edges[k - 1]))
            return fail(WPT_ERR_INVALID_ARGUMENT, "transient film: bin edges must increase (edge " + std::to_string(k) + ")");
    }
    /* the kernels' first guess of a bin: uniform spacing between the first and the last finite edge */
    const uint32_t lastFinite = std::isinf(edges[binCount]) ? binCount - 1 : binCount;
    float scale = lastFinite > 0 ? float(lastFinite) / (edges[lastFinite] - edges[0]) : 0.0f;
    bv = wptk::BinsView{};
    bv.binCount = binCount;
    bv.guessScale = std::isfinite(scale) ? scale : 0.0f;
    return WPT_OK;
}

/* One launch into planes of accumulated values, the transient film's or the time-of-flight sensor's.  `table`, the sensor's
 * words, goes to the device as rq.bins.edges; where the kernels accumulate into the planes (`accumulated`), the planes' block is
 * zeroed before the render and scaled by 1 / samples behind it, all in stream order.  rq.bins.bins is plane 0's pixel 0 with
 * rq.bins.stride floats between planes (a full frame's, or a block's behind a biased pointer); what: the sensor, for messages. */
wpt_status planesLaunch(LaunchRequest rq, const float* table, size_t tableFloats, bool accumulated, const char* what)
{
    const wptk::BinsView& bv = rq.bins;
    hipStream_t stream = static_cast<hipStream_t>(rq.stream);
    float* dTable = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&dTable), tableFloats * sizeof(float), stream));
    hipError_t e = hipMemcpyAsync(dTable, table, tableFloats * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && accumulated)
        e = hipMemset2DAsync(bv.bins + size_t(rq.blockStart) * 3, bv.stride * sizeof(float), 0, size_t(rq.blockSize) * 3 * sizeof(float), bv.binCount,
                stream);
    if (e != hipSuccess) {
        (void)hipFreeAsync(dTable, stream);
        return fail(WPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    rq.bins.edges = dTable;
    wpt_status st = renderLaunch(rq);
    if (st == WPT_OK && accumulated) {
        const uint64_t n = uint64_t(rq.blockSize) * 3 * bv.binCount;
        const uint32_t blocks = uint32_t(std::min<uint64_t>((n + 255) / 256, 65536));
        hipLaunchKernelGGL(wpt_transient_finish_kernel, dim3(blocks), dim3(256), 0, stream, bv.bins, bv.stride, rq.blockStart, rq.blockSize,
                bv.binCount, 1.0f / float(rq.samplesSqrt * rq.samplesSqrt));
        e = hipGetLastError();
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    (void)hipFreeAsync(dTable, stream);
    return st;
}

/* one transient launch; `bins` and `stride` as planesLaunch takes them */
wpt_status transientLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const float* edges, uint32_t binCount,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* frame, float* bins,
        size_t stride, hipStream_t stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame, stream };
    WPT_TRY(transientEdges(edges, binCount, rq.bins));
    if (!scene || !camera || !params || !bins)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    rq.sensor = wptk::SENSOR_TRANSIENT;
    rq.bins.bins = bins;
    rq.bins.stride = stride;
    rq.bins.width = width;
    return planesLaunch(rq, edges, size_t(binCount) + 1, true, "transient film");
}

/* refuses a bad light-groups table; fills what the kernels need of a good one but the device copy of the table */
wpt_status lightGroupsTable(const uint8_t* groupOfMaterial, uint32_t materialCount, uint32_t groupCount, uint32_t envGroup, wptk::BinsView& bv)
{
    uint32_t at = 0;
    switch (wptmix::checkTable(groupOfMaterial, materialCount, groupCount, envGroup, &at)) {
    case wptmix::TABLE_OK:
        break;
    case wptmix::TABLE_NULL:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the table of the materials' groups is NULL");
    case wptmix::TABLE_GROUP_COUNT:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: group count must lie in 1 .. " + std::to_string(WPT_LIGHT_GROUPS_MAX));
    case wptmix::TABLE_ENTRY:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: material " + std::to_string(at) + " has group " + std::to_string(groupOfMaterial[at])
                + ", which is neither below the group count " + std::to_string(groupCount) + " nor WPT_LIGHT_GROUP_NONE");
    case wptmix::TABLE_ENV_GROUP:
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the environment's group " + std::to_string(envGroup)
                + " is neither below the group count " + std::to_string(groupCount) + " nor WPT_LIGHT_GROUP_NONE");
    }
    bv = wptk::BinsView{};
    bv.binCount = groupCount;
    bv.rule = wptk::BINS_BY_EMITTER | envGroup;
    return WPT_OK;
}

/* one light-groups launch: a launch of the transient film's kernels whose BinsView says "plane by emitter"; `planes` and
 * `stride` as planesLaunch takes them.  The table travels as the sensor's words, padded to whole floats with NONE. */
wpt_status lightGroupsLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const uint8_t* groupOfMaterial,
        uint32_t materialCount, uint32_t groupCount, uint32_t envGroup, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size, float* frame, float* planes, size_t stride, hipStream_t stream)
{
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, frame, stream };
    WPT_TRY(lightGroupsTable(groupOfMaterial, materialCount, groupCount, envGroup, rq.bins));
    if (!scene || !camera || !params || !planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (materialCount != uint32_t(scene->view.materialCount))
        return fail(WPT_ERR_INVALID_ARGUMENT, "light groups: the table has " + std::to_string(materialCount) + " materials, the scene "
                + std::to_string(uint32_t(scene->view.materialCount)));
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    rq.sensor = wptk::SENSOR_TRANSIENT;
    rq.bins.bins = planes;
    rq.bins.stride = stride;
    rq.bins.width = width;
    std::vector<float> words((size_t(materialCount) + 3) / 4 + 1);
    memset(words.data(), 0xff, words.size() * sizeof(float));
    memcpy(words.data(), groupOfMaterial, materialCount);
    return planesLaunch(rq, words.data(), words.size(), true, "light groups");
}

/* the mix of planes (wpt_lightmix.h): one thread per value */
__global__ void wpt_lightmix_kernel(const float* planes, uint32_t planeCount, size_t stride, uint64_t values, const float* weights, float* out)
{
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < values)
        out[i] = wptmix::mixValue(planes, planeCount, stride, weights, size_t(i));
}

/* what a mix is refused for, on the device or on the host */
wpt_status mixCheck(const void* planes, uint32_t planeCount, uint64_t stride, uint64_t pixels, const void* weights, const void* out)
{
    if (!planes || !weights || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: NULL argument");
    if (planeCount == 0 || planeCount > wptmix::PLANES_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: plane count must lie in 1 .. " + std::to_string(uint32_t(wptmix::PLANES_MAX)));
    if (pixels == 0 || pixels > 0x7fffffffull * 256ull / 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: bad pixel count");
    if (planeCount > 1 && stride < pixels * 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: the planes overlap (stride below pixels * 3)");
    return WPT_OK;
}

/* what a denoiser call is refused for, on the device or on the host; fills in the defaults and the filter's own parameters */
wpt_status denoiseCheck(const void* frame, const void* moments, const void* samplesSqrt, const void* positions, const void* normals,
        const void* materials, uint32_t width, uint32_t height, const wpt_denoise_params* params, const void* out, const void* variance,
        wptdn::Params& filter, uint32_t& iterations)
{
    if (!frame || !moments || !samplesSqrt || !positions || !normals || !materials)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: an input is NULL");
    if (!out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame is NULL");
    if (width == 0 || height == 0 || width > wptdn::SIDE_MAX || height > wptdn::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: width and height must lie in 1 .. " + std::to_string(uint32_t(wptdn::SIDE_MAX)));
    const wpt_denoise_params defaults = { 1.0f, 0.1f, 7u, 5u };
    const wpt_denoise_params& p = params ? *params : defaults;
    if (p.iterations > WPT_DENOISE_MAX_ITERATIONS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: iterations must lie in 0 .. " + std::to_string(WPT_DENOISE_MAX_ITERATIONS));
    if (p.normal_log2 > WPT_DENOISE_MAX_NORMAL_LOG2)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: normal_log2 must lie in 0 .. " + std::to_string(WPT_DENOISE_MAX_NORMAL_LOG2));
    if (!(std::isfinite(p.sigma_l) && p.sigma_l > 0.0f) || !(std::isfinite(p.sigma_z) && p.sigma_z > 0.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: sigma_l and sigma_z must be finite and positive");
    /* the byte ranges of the arrays: an output may overlap neither an input nor the other output */
    const size_t pixels = size_t(width) * height;
    const struct { const void* at; size_t bytes; } in[] = { { frame, pixels * 12 }, { moments, pixels * 12 }, { samplesSqrt, pixels * 2 },
        { positions, pixels * 12 }, { normals, pixels * 12 }, { materials, pixels * 4 }, { variance, pixels * 4 } };
    const auto overlap = [](const void* a, size_t an, const void* b, size_t bn) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
        return x < y + bn && y < x + an;
    };
    for (size_t k = 0; k < sizeof(in) / sizeof(in[0]); k++) {
        if (in[k].at && overlap(out, pixels * 12, in[k].at, in[k].bytes))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame aliases another array of the call");
        if (variance && k < 6 && overlap(variance, pixels * 4, in[k].at, in[k].bytes))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the variance plane aliases another array of the call");
    }
    filter.sigmaL = p.sigma_l;
    filter.sigmaZ2 = p.sigma_z * p.sigma_z;
    filter.normalLog2 = p.normal_log2;
    iterations = p.iterations;
    return WPT_OK;
}

/* the same for the demodulated form: the two planes of the first-hit colours beside the inputs, and the floor of the albedo */
wpt_status denoiseDemodulatedCheck(const void* frame, const void* moments, const void* samplesSqrt, const void* positions, const void* normals,
        const void* materials, const void* albedo, const void* emission, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float& albedoFloor, const void* out, const void* variance, wptdn::Params& filter, uint32_t& iterations)
{
    if (!albedo || !emission)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the albedo or the emission plane is NULL");
    if (!std::isfinite(albedoFloor))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: albedo_floor must be finite (<= 0: the default)");
    WPT_TRY(denoiseCheck(frame, moments, samplesSqrt, positions, normals, materials, width, height, params, out, variance, filter, iterations));
    const size_t pixels = size_t(width) * height;
    const auto overlap = [](const void* a, size_t an, const void* b, size_t bn) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
        return x < y + bn && y < x + an;
    };
    for (const void* plane : { albedo, emission }) {
        if (overlap(out, pixels * 12, plane, pixels * 12))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame aliases another array of the call");
        if (variance && overlap(variance, pixels * 4, plane, pixels * 12))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the variance plane aliases another array of the call");
    }
    if (albedoFloor <= 0.0f)
        albedoFloor = wptdn::k_albedoFloorDefault;
    return WPT_OK;
}

/* what a call of the image operations (wpt_image_ops.h) is refused for, on the device or on the host: `what` names the call,
 * the output holds outWidth x outHeight x outComps floats */
wpt_status imageOpCheck(const char* what, const void* image, uint32_t width, uint32_t height, uint32_t comps, const void* out,
        uint32_t outWidth, uint32_t outHeight, uint32_t outComps)
{
    const std::string name(what);
    if (!image || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the image or the output is NULL");
    if (width == 0 || height == 0 || width > wptio::SIDE_MAX || height > wptio::SIDE_MAX || outWidth == 0 || outHeight == 0
            || outWidth > wptio::SIDE_MAX || outHeight > wptio::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": width and height must lie in 1 .. " + std::to_string(uint32_t(wptio::SIDE_MAX)));
    if (comps < 1 || comps > wptio::COMPONENTS_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the image must have 1 .. 4 components");
    const size_t inBytes = size_t(width) * height * comps * sizeof(float), outBytes = size_t(outWidth) * outHeight * outComps * sizeof(float);
    const uintptr_t x = reinterpret_cast<uintptr_t>(image), y = reinterpret_cast<uintptr_t>(out);
    if (x < y + outBytes && y < x + inBytes)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the output overlaps the image");
    return WPT_OK;
}

/* the lens of a warp or of a distance image: only the distortion part of the camera record is read */
wpt_status imageOpLens(const char* what, const wpt_camera* camera, wptlens::Coeffs& lens)
{
    if (!camera)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(what) + ": the camera is NULL");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown distortion type " + std::to_string(camera->distortion_type));
    lens = wptlens::coeffs(*camera);
    return WPT_OK;
}

wpt_status despeckleCheck(const void* rgb, uint32_t width, uint32_t height, uint32_t comps, float minFactor, const void* out)
{
    if (rgb && out && comps != 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle: the image must have 3 components");
    WPT_TRY(imageOpCheck("despeckle", rgb, width, height, 3, out, width, height, 3));
    if (!std::isfinite(minFactor))
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle: min_factor must be finite");
    return WPT_OK;
}

/* -1: as built (WPT_DESPECKLE_TILE), 0: gather, 1: tile; wpt_set_despeckle_form */
int g_despeckleForm = -1;

bool despeckleTile()
{
    return g_despeckleForm < 0 ? wptk::despeckleTileByDefault() : g_despeckleForm != 0;
}

/* what a batch of views is refused for before anything needs the scene or a device */
wpt_status viewsCheck(const wpt_camera* cameras, uint32_t viewCount, const void* frames, uint32_t width, uint32_t height)
{
    if (viewCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: view_count is 0");
    if (!cameras)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: cameras are NULL");
    if (!frames)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: frames are NULL");
    for (uint32_t v = 0; v < viewCount; v++)
        if (cameras[v].animation < -1)
            return fail(WPT_ERR_INVALID_ARGUMENT, "views: camera " + std::to_string(v) + " refers to an animation outside the scene's array");
    /* the kernels index the batch's pixels, and hand them out from the pixel pool, in 32 bits */
    if (uint64_t(viewCount) * width * height > WPT_VIEWS_MAX_PIXELS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "views: view_count * width * height exceeds " + std::to_string(WPT_VIEWS_MAX_PIXELS) + " pixels");
    return WPT_OK;
}

/* what a split render is refused for before anything needs the scene or a device */
wpt_status splitCheck(const wpt_camera* camera, uint32_t width, uint32_t height, uint32_t firstStream, uint32_t streamCount, const void* frame)
{
    if (streamCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: stream_count is 0");
    if (!camera)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: the camera is NULL");
    if (!frame)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: the frame is NULL");
    if (uint64_t(streamCount) * width * height > WPT_VIEWS_MAX_PIXELS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: stream_count * width * height exceeds " + std::to_string(WPT_VIEWS_MAX_PIXELS) + " pixels");
    if (uint64_t(firstStream) + streamCount > 0x100000000ull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split: first_stream + stream_count exceeds 2^32");
    return WPT_OK;
}

/* what a mean of planes is refused for, on the device or on the host */
wpt_status meanCheck(const void* planes, uint32_t planeCount, uint64_t stride, uint64_t pixels, const void* mean)
{
    if (!planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: the planes are NULL");
    if (!mean)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: mean_out is NULL");
    if (planeCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: plane_count is 0");
    if (pixels == 0 || pixels > wptk::STREAMS_MAX_VALUES / 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: bad pixel count");
    if (planeCount > 1 && stride < pixels * 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: the planes overlap (stride below pixels * 3)");
    return WPT_OK;
}

/* what a merge of two means is refused for, on the device or on the host */
wpt_status mergeCheck(const void* a, uint32_t countA, const void* b, uint32_t countB, uint64_t values, const void* out)
{
    if (!a || !b || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: NULL argument");
    if (uint64_t(countA) + countB == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: count_a + count_b is 0");
    if (values == 0 || values > wptk::STREAMS_MAX_VALUES)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: bad value count");
    return WPT_OK;
}

/* what a batch of views is refused for: viewsCheck, and with the scene at hand what needs it */
wpt_status viewsChecked(const wpt_scene* scene, const wpt_camera* cameras, uint32_t viewCount, const wpt_params* params, uint32_t width,
        uint32_t height, uint32_t samplesSqrt, const void* frames)
{
    WPT_TRY(viewsCheck(cameras, viewCount, frames, width, height));
    if (!scene || !params)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t v = 0; v < viewCount; v++)
        if (cameras[v].animation >= int32_t(scene->animationCount))
            return fail(WPT_ERR_INVALID_ARGUMENT, "views: camera " + std::to_string(v) + " refers to an animation outside the scene's array");
    return checkFrameBlock(width, height, &samplesSqrt, 0, 0);
}

/* the launch of a batch whose cameras and stream numbers (or NULL: all 0) are in device memory, written in stream order before
 * it; camerasHost: the same cameras, read for the launch's features */
wpt_status viewsLaunch(wpt_scene* scene, const wpt_camera* camerasHost, const wpt_camera* camerasDevice, const uint32_t* streamsDevice,
        uint32_t viewCount, const wpt_params* params, uint32_t width, uint32_t height, uint32_t samplesSqrt, float* frames,
        wpt_counters* counters, void* hipStream)
{
    LaunchRequest rq = { scene, camerasHost, params, width, height, samplesSqrt, 0, viewCount * width * height, frames, hipStream };
    rq.counters = counters;
    rq.sensor = wptk::SENSOR_VIEWS;
    rq.views = { camerasDevice, width * height, viewCount, streamsDevice };
    return renderLaunch(rq);
}

/* what an adaptive render is refused for before anything needs the scene or a device (every 16-bit count is valid) */
wpt_status adaptiveCheck(uint32_t width, uint32_t height, const void* map, uint32_t blockStart, uint32_t blockSize, const void* frame)
{
    if (!map)
        return fail(WPT_ERR_INVALID_ARGUMENT, "adaptive: the sample-count map is NULL");
    if (!frame)
        return fail(WPT_ERR_INVALID_ARGUMENT, "adaptive: the frame is NULL");
    return checkFrameBlock(width, height, nullptr, blockStart, blockSize, 1, "adaptive: ");
}

/* refuses a bad time-of-flight call before a device is needed */
wpt_status tofCheck(const void* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor, const void* planes)
{
    if (!scene || !camera || !params || !sensor || !planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: NULL argument");
    if (sensor->phase_count == 0 || sensor->phase_count > WPT_TOF_MAX_PHASES)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: phase count must lie in 1 .. " + std::to_string(WPT_TOF_MAX_PHASES));
    bool finite = std::isfinite(sensor->pixel_area) && std::isfinite(sensor->exposure_time) && std::isfinite(sensor->contrast)
            && std::isfinite(sensor->frac_modfreq_c);
    for (uint32_t j = 0; j < sensor->phase_count; j++)
        finite = finite && std::isfinite(sensor->tau[j]);
    if (!finite)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: a sensor value is NaN or infinite");
    if (!(sensor->contrast >= 0.0f && sensor->contrast <= 1.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: contrast must lie in [0, 1]");
    if (params->min_dist_to_light != 0.0f || params->max_dist_to_light != FLT_MAX || params->min_path_len != 0.0f || params->max_path_len != FLT_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: it has no gates (the distance and path length gates must be the defaults)");
    return WPT_OK;
}

/* one time-of-flight launch.  One phase: the kernel keeps the taps in the pixel's accumulator and writes the plane as an RGB
 * launch writes its frame.  Several: the planes' block is zeroed, rendered into and scaled, all in stream order, as the
 * transient film's.  `planes` is plane 0's pixel 0 with `stride` floats between planes. */
wpt_status tofLaunch(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* planes, size_t stride,
        hipStream_t stream)
{
    WPT_TRY(tofCheck(scene, camera, params, sensor, planes));
    const wpt_status inFrame = checkFrameBlock(width, height, &samples_sqrt, block_start, block_size);
    if (inFrame != WPT_OK || block_size == 0)
        return inFrame;
    const uint32_t phases = sensor->phase_count;
    float consts[wpttof::C_TAU + WPT_TOF_MAX_PHASES] = {};
    consts[wpttof::C_PIXEL_AREA] = sensor->pixel_area;
    consts[wpttof::C_EXPOSURE_TIME] = sensor->exposure_time;
    consts[wpttof::C_CONTRAST] = sensor->contrast;
    consts[wpttof::C_FRAC_MODFREQ_C] = sensor->frac_modfreq_c;
    for (uint32_t j = 0; j < phases; j++)
        consts[wpttof::C_TAU + j] = sensor->tau[j];
    LaunchRequest rq = { scene, camera, params, width, height, samples_sqrt, block_start, block_size, phases == 1 ? planes : nullptr, stream };
    rq.sensor = wptk::SENSOR_TOF;
    rq.bins.bins = planes;
    rq.bins.stride = stride;
    rq.bins.binCount = phases;
    rq.bins.width = width;
    return planesLaunch(rq, consts, sizeof(consts) / sizeof(consts[0]), phases > 1, "time-of-flight sensor");
}

} /* namespace */

extern "C" {

wpt_status wpt_render_transient_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const float* edges_host, uint32_t bin_count, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start,
        uint32_t block_size, float* frame_device, float* bins_device, void* hip_stream)
{
    return transientLaunch(scene, camera, params, edges_host, bin_count, width, height, samples_sqrt, block_start, block_size,
            frame_device, bins_device, size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_transient_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const float* edges_host, uint32_t bin_count, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start,
        uint32_t block_size, float* block_rgb, float* block_bins)
{
    wptk::BinsView bv;
    WPT_TRY(transientEdges(edges_host, bin_count, bv));
    if (!block_bins)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_bins is NULL");
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block, bins;
    if (block_rgb)
        HIP_TRY(block.allocatePixels(block_size));
    const hipError_t e = bins.allocatePixels(block_size, bin_count);
    if (e != hipSuccess)
        return fail(WPT_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    return finishStaged(transientLaunch(scene, camera, params, edges_host, bin_count, width, height, samples_sqrt, block_start, block_size,
            block.biased(block_start), bins.biased(block_start), size_t(block_size) * 3, nullptr), scene, block, block_rgb, &bins, block_bins);
}

wpt_status wpt_render_light_groups_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count, uint32_t env_group, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* frame_device, float* planes_device, void* hip_stream)
{
    return lightGroupsLaunch(scene, camera, params, group_of_material, material_count, group_count, env_group, width, height, samples_sqrt,
            block_start, block_size, frame_device, planes_device, size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_light_groups_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count, uint32_t env_group, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_rgb, float* block_planes)
{
    wptk::BinsView bv;
    WPT_TRY(lightGroupsTable(group_of_material, material_count, group_count, env_group, bv));
    if (!block_planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "block_planes is NULL");
    if (block_size == 0)
        return WPT_OK;
    StagedBlock block, planes;
    if (block_rgb)
        HIP_TRY(block.allocatePixels(block_size));
    const hipError_t e = planes.allocatePixels(block_size, group_count);
    if (e != hipSuccess)
        return fail(WPT_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    return finishStaged(lightGroupsLaunch(scene, camera, params, group_of_material, material_count, group_count, env_group, width, height,
            samples_sqrt, block_start, block_size, block.biased(block_start), planes.biased(block_start), size_t(block_size) * 3, nullptr),
            scene, block, block_rgb, &planes, block_planes);
}

wpt_status wpt_postproc_mix_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_device, void* hip_stream)
{
    WPT_TRY(mixCheck(planes_device, plane_count, stride, pixels, weights_host, out_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t weightBytes = size_t(plane_count) * 3 * sizeof(float);
    float* dWeights = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&dWeights), weightBytes, stream));
    hipError_t e = hipMemcpyAsync(dWeights, weights_host, weightBytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(wpt_lightmix_kernel, dim3(uint32_t((pixels * 3 + 255) / 256)), dim3(256), 0, stream, planes_device, plane_count,
                size_t(stride), pixels * 3, dWeights, out_device);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(dWeights, stream);
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("mix of planes: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_mix_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_host)
{
    WPT_TRY(mixCheck(planes_host, plane_count, stride, pixels, weights_host, out_host));
    wptmix::mixHost(planes_host, plane_count, size_t(stride), pixels, weights_host, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_denoise(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_device, float* variance_device, void* hip_stream)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseCheck(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device, materials_device, width, height,
            params, out_device, variance_device, filter, iterations));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    wptdn::Rec* scratch = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), size_t(width) * height * 4 * sizeof(wptdn::Rec), stream));
    const hipError_t e = wptk::launchDenoise(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device,
            materials_device, width, height, filter, iterations, scratch, out_device, variance_device, stream);
    (void)hipFreeAsync(scratch, stream);
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("denoise: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_denoise_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_host, float* variance_host)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseCheck(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, width, height, params,
            out_host, variance_host, filter, iterations));
    std::vector<wptdn::Rec> scratch(size_t(width) * height * 4);
    wptdn::denoiseHost(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, width, height, filter,
            iterations, scratch.data(), out_host, variance_host);
    return WPT_OK;
}

const char* wpt_postproc_denoise_form(uint32_t step)
{
    return wptk::denoiseFormOfStep(step);
}

wpt_status wpt_postproc_denoise_demodulated(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, const float* albedo_device,
        const float* emission_device, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_device, float* variance_device, void* hip_stream)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseDemodulatedCheck(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device, materials_device,
            albedo_device, emission_device, width, height, params, albedo_floor, out_device, variance_device, filter, iterations));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    wptdn::Rec* scratch = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), size_t(width) * height * 4 * sizeof(wptdn::Rec), stream));
    const hipError_t e = wptk::launchDenoiseDemodulated(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device,
            materials_device, albedo_device, emission_device, width, height, filter, iterations, albedo_floor, scratch, out_device,
            variance_device, stream);
    (void)hipFreeAsync(scratch, stream);
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("denoise: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_denoise_demodulated_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, const float* albedo_host,
        const float* emission_host, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_host, float* variance_host)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseDemodulatedCheck(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, albedo_host,
            emission_host, width, height, params, albedo_floor, out_host, variance_host, filter, iterations));
    std::vector<wptdn::Rec> scratch(size_t(width) * height * 4);
    wptdn::denoiseDemodulatedHost(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, albedo_host,
            emission_host, width, height, filter, iterations, albedo_floor, scratch.data(), out_host, variance_host);
    return WPT_OK;
}

wpt_status wpt_postproc_resample(const float* image_device, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_device, void* hip_stream)
{
    WPT_TRY(imageOpCheck("resample", image_device, width, height, components, out_device, new_width, new_height, components));
    const wptio::Image img = { image_device, width, height, components };
    const hipError_t e = wptk::launchResample(img, new_width, new_height, out_device, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("resample: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_resample_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_host)
{
    WPT_TRY(imageOpCheck("resample", image_host, width, height, components, out_host, new_width, new_height, components));
    const wptio::Image img = { image_host, width, height, components };
    wptio::resampleHost(img, new_width, new_height, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_lens_warp(const float* image_device, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_device, void* hip_stream)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("lens warp", image_device, width, height, components, out_device, width, height, components));
    WPT_TRY(imageOpLens("lens warp", camera, lens));
    const wptio::Image img = { image_device, width, height, components };
    const hipError_t e = wptk::launchLensWarp(img, lens, forward != 0, out_device, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("lens warp: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_lens_warp_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_host)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("lens warp", image_host, width, height, components, out_host, width, height, components));
    WPT_TRY(imageOpLens("lens warp", camera, lens));
    const wptio::Image img = { image_host, width, height, components };
    wptio::warpHost(img, lens, forward != 0, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_despeckle(const float* rgb_device, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_device, void* hip_stream)
{
    WPT_TRY(despeckleCheck(rgb_device, width, height, components, min_factor, out_device));
    const hipError_t e = wptk::launchDespeckle(rgb_device, width, height, min_factor, despeckleTile(), out_device, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("despeckle: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_despeckle_host(const float* rgb_host, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_host)
{
    WPT_TRY(despeckleCheck(rgb_host, width, height, components, min_factor, out_host));
    wptio::despeckleHost(rgb_host, width, height, min_factor, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_distance_to_coords(const float* distances_device, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_device, void* hip_stream)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("distance to coordinates", distances_device, width, height, components, coords_device, width, height, 3));
    WPT_TRY(imageOpLens("distance to coordinates", camera, lens));
    const wptio::Image img = { distances_device, width, height, components };
    const hipError_t e = wptk::launchDistanceToCoords(img, lens, pmd_space != 0, coords_device, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("distance to coordinates: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_distance_to_coords_host(const float* distances_host, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_host)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("distance to coordinates", distances_host, width, height, components, coords_host, width, height, 3));
    WPT_TRY(imageOpLens("distance to coordinates", camera, lens));
    const wptio::Image img = { distances_host, width, height, components };
    wptio::coordsHost(img, lens, pmd_space != 0, coords_host);
    return WPT_OK;
}

const char* wpt_postproc_despeckle_form(void)
{
    return despeckleTile() ? "tile" : "gather";
}

wpt_status wpt_set_despeckle_form(int form)
{
    if (form < -1 || form > 1)
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle form: -1 (as built), 0 (gather) or 1 (tile)");
    g_despeckleForm = form;
    return WPT_OK;
}

void wpt_postproc_image_ops_tile(uint32_t* width, uint32_t* height)
{
    if (width)
        *width = wptk::IMAGE_OPS_TILE_W;
    if (height)
        *height = wptk::IMAGE_OPS_TILE_H;
}

wpt_status wpt_render_view_streams_device(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_device, wpt_counters* counters_device,
        void* hip_stream)
{
    WPT_TRY(viewsChecked(scene, cameras_host, view_count, params, width, height, samples_sqrt, frames_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* the cameras, and behind them the views' stream numbers, go to device memory once per batch, in stream order */
    const size_t camBytes = size_t(view_count) * sizeof(wpt_camera), streamBytes = streams_host ? size_t(view_count) * sizeof(uint32_t) : 0;
    static_assert(sizeof(wpt_camera) % alignof(uint32_t) == 0, "the stream numbers lie behind the cameras");
    wpt_camera* dCams = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&dCams), camBytes + streamBytes, stream));
    uint32_t* dStreams = streams_host ? reinterpret_cast<uint32_t*>(dCams + view_count) : nullptr;
    hipError_t e = hipMemcpyAsync(dCams, cameras_host, camBytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && streams_host)
        e = hipMemcpyAsync(dStreams, streams_host, streamBytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
        (void)hipFreeAsync(dCams, stream);
        return fail(WPT_ERR_HIP, std::string("views: ") + hipGetErrorString(e));
    }
    const wpt_status st = viewsLaunch(scene, cameras_host, dCams, dStreams, view_count, params, width, height, samples_sqrt, frames_device,
            counters_device, hip_stream);
    (void)hipFreeAsync(dCams, stream);
    return st;
}

wpt_status wpt_render_view_streams(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host)
{
    WPT_TRY(viewsCheck(cameras_host, view_count, frames_host, width, height));
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock frames;
    HIP_TRY(frames.allocatePixels(size_t(view_count) * width * height));
    return finishStaged(wpt_render_view_streams_device(scene, cameras_host, streams_host, view_count, params, width, height, samples_sqrt,
            frames.biased(0), nullptr, nullptr), scene, frames, frames_host);
}

wpt_status wpt_render_views_device(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_device, wpt_counters* counters_device, void* hip_stream)
{
    return wpt_render_view_streams_device(scene, cameras_host, nullptr, view_count, params, width, height, samples_sqrt, frames_device,
            counters_device, hip_stream);
}

wpt_status wpt_render_views(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host)
{
    return wpt_render_view_streams(scene, cameras_host, nullptr, view_count, params, width, height, samples_sqrt, frames_host);
}

wpt_status wpt_render_split_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_device, float* moments_device,
        wpt_counters* counters_device, void* hip_stream)
{
    WPT_TRY(splitCheck(camera, width, height, first_stream, stream_count, frame_device));
    /* the streams are a batch of views of one camera: view i is stream first_stream + i (the host's copies are read for the
     * launch's checks and features only, before this returns) */
    const std::vector<wpt_camera> cameras(stream_count, *camera);
    WPT_TRY(viewsChecked(scene, cameras.data(), stream_count, params, width, height, stream_samples_sqrt, frame_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* one allocation in stream order: the streams' frames, then their cameras and numbers, which a kernel writes (nothing
     * of the host's is read once the call has returned) */
    const size_t values = size_t(width) * height * 3, frameBytes = values * stream_count * sizeof(float);
    const size_t camBytes = size_t(stream_count) * sizeof(wpt_camera);
    static_assert(alignof(wpt_camera) <= alignof(float), "the cameras lie behind the streams' frames");
    float* scratch = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), frameBytes + camBytes + size_t(stream_count) * sizeof(uint32_t), stream));
    wpt_camera* dCams = reinterpret_cast<wpt_camera*>(scratch + values * stream_count);
    uint32_t* dStreams = reinterpret_cast<uint32_t*>(dCams + stream_count);
    wpt_status st = WPT_OK;
    hipError_t e = wptk::launchFillStreamViews(*camera, first_stream, stream_count, dCams, dStreams, stream);
    if (e == hipSuccess) {
        st = viewsLaunch(scene, cameras.data(), dCams, dStreams, stream_count, params, width, height, stream_samples_sqrt, scratch,
                counters_device, hip_stream);
        if (st == WPT_OK)
            e = wptk::launchMeanPlanes(scratch, stream_count, values, values, frame_device, moments_device, stream);
    }
    (void)hipFreeAsync(scratch, stream);
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("split: ") + hipGetErrorString(e));
    return st;
}

wpt_status wpt_render_split(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_host, float* moments_host)
{
    WPT_TRY(splitCheck(camera, width, height, first_stream, stream_count, frame_host));
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    StagedBlock frame, moments;
    HIP_TRY(frame.allocatePixels(size_t(width) * height));
    if (moments_host)
        HIP_TRY(moments.allocatePixels(size_t(width) * height));
    return finishStaged(wpt_render_split_device(scene, camera, params, width, height, stream_samples_sqrt, first_stream, stream_count,
            frame.biased(0), moments.biased(0), nullptr, nullptr), scene, frame, frame_host, &moments, moments_host);
}

wpt_status wpt_postproc_mean_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_device, float* moment_out_device, void* hip_stream)
{
    WPT_TRY(meanCheck(planes_device, plane_count, stride, pixels, mean_out_device));
    const hipError_t e = wptk::launchMeanPlanes(planes_device, plane_count, size_t(stride), pixels * 3, mean_out_device, moment_out_device,
            static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("mean of planes: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_mean_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_host, float* moment_out_host)
{
    WPT_TRY(meanCheck(planes_host, plane_count, stride, pixels, mean_out_host));
    wptstr::meanHost(planes_host, plane_count, size_t(stride), pixels * 3, mean_out_host, moment_out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_merge_means(const float* a_device, uint32_t count_a, const float* b_device, uint32_t count_b, uint64_t values,
        float* out_device, void* hip_stream)
{
    WPT_TRY(mergeCheck(a_device, count_a, b_device, count_b, values, out_device));
    const hipError_t e = wptk::launchMergeMeans(a_device, count_a, b_device, count_b, values, out_device, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess)
        return fail(WPT_ERR_HIP, std::string("merge of means: ") + hipGetErrorString(e));
    return WPT_OK;
}

wpt_status wpt_postproc_merge_means_host(const float* a_host, uint32_t count_a, const float* b_host, uint32_t count_b, uint64_t values,
        float* out_host)
{
    WPT_TRY(mergeCheck(a_host, count_a, b_host, count_b, values, out_host));
    wptstr::mergeHost(a_host, count_a, b_host, count_b, values, out_host);
    return WPT_OK;
}

wpt_status wpt_split_plan(uint64_t pixels, uint32_t samples_sqrt, uint32_t lanes, uint32_t* stream_count, uint32_t* stream_samples_sqrt)
{
    if (!stream_count || !stream_samples_sqrt)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split plan: NULL argument");
    if (!wptstr::splitPlan(pixels, samples_sqrt, lanes, stream_count, stream_samples_sqrt))
        return fail(WPT_ERR_INVALID_ARGUMENT, "split plan: pixels, samples_sqrt and lanes must be above 0");
    return WPT_OK;
}

wpt_status wpt_device_lanes(int device, uint32_t* lanes)
{
    if (!lanes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "device lanes: NULL argument");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    *lanes = uint32_t(prop.multiProcessorCount) * 1024u;
    return WPT_OK;
}

wpt_status wpt_render_adaptive_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_device, uint32_t block_start, uint32_t block_size,
        float* frame_device, float* moments_device, void* hip_stream)
{
    WPT_TRY(adaptiveCheck(width, height, samples_sqrt_device, block_start, block_size, frame_device));
    /* (the launch's own samples_sqrt is unused by the adaptive kernels: 1 passes renderLaunch's checks) */
    LaunchRequest rq = { scene, camera, params, width, height, 1, block_start, block_size, frame_device, hip_stream };
    rq.sensor = wptk::SENSOR_ADAPTIVE;
    rq.adaptive = { samples_sqrt_device, moments_device };
    return renderLaunch(rq);
}

wpt_status wpt_render_adaptive_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_host, uint32_t block_start, uint32_t block_size,
        float* block_rgb, float* block_moments)
{
    WPT_TRY(adaptiveCheck(width, height, samples_sqrt_host, block_start, block_size, block_rgb));
    if (block_size == 0)
        return WPT_OK;
    /* device memory for the block only, behind pointers biased so that pixel `block_start` lands at offset 0; the caller's
     * values go there first, so that the pixels with n = 0 come back as they were */
    StagedBlock map, block, moments;
    hipError_t e = map.allocate(size_t(block_size) * sizeof(uint16_t));
    if (e == hipSuccess)
        e = block.allocatePixels(block_size);
    if (e == hipSuccess && block_moments)
        e = moments.allocatePixels(block_size);
    if (e == hipSuccess)
        e = map.upload(samples_sqrt_host + block_start);
    if (e == hipSuccess)
        e = block.upload(block_rgb);
    if (e == hipSuccess && block_moments)
        e = moments.upload(block_moments);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("adaptive: ") + hipGetErrorString(e));
    return finishStaged(wpt_render_adaptive_block_device(scene, camera, params, width, height, static_cast<uint16_t*>(map.device) - block_start,
            block_start, block_size, block.biased(block_start), moments.biased(block_start), nullptr), scene,
            block, block_rgb, &moments, block_moments);
}

wpt_status wpt_render_tof_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* planes_device,
        void* hip_stream)
{
    return tofLaunch(scene, camera, params, sensor, width, height, samples_sqrt, block_start, block_size, planes_device,
            size_t(width) * height * 3, static_cast<hipStream_t>(hip_stream));
}

wpt_status wpt_render_tof_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_tof_sensor* sensor,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, float* block_planes)
{
    WPT_TRY(tofCheck(scene, camera, params, sensor, block_planes));
    if (block_size == 0)
        return WPT_OK;
    StagedBlock planes;
    HIP_TRY(planes.allocatePixels(block_size, sensor->phase_count));
    return finishStaged(tofLaunch(scene, camera, params, sensor, width, height, samples_sqrt, block_start, block_size, planes.biased(block_start),
            size_t(block_size) * 3, nullptr), scene, planes, block_planes);
}

wpt_status wpt_tof_accumulate_host(const wpt_tof_sensor* sensor, uint32_t phase, float radiance_w, float opl_w, int is_tof_light, float acc[3])
{
    if (!sensor || !acc)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: NULL argument");
    if (sensor->phase_count == 0 || sensor->phase_count > WPT_TOF_MAX_PHASES || phase >= sensor->phase_count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "time-of-flight sensor: phase outside the sensor's phase count (1 .. " + std::to_string(WPT_TOF_MAX_PHASES) + ")");
    const float energy = wpttof::energy(sensor->pixel_area, sensor->exposure_time, radiance_w);
    const float t = is_tof_light ? wpttof::modulation(sensor->contrast, sensor->frac_modfreq_c, sensor->tau[phase], opl_w) : 0.0f;
    wpttof::add(energy, t, acc[0], acc[1], acc[2]);
    return WPT_OK;
}

wpt_status wpt_ground_truth_device(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_device[WPT_GT_ARRAY_COUNT], void* hip_stream)
{
    if (!scene || !camera || !params || !arrays_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width == 0 || height == 0 || uint64_t(width) * height > 0xffffffffull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (camera->surround_mode > WPT_SURROUND_360)
        return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
    if ((arrays_device[WPT_GT_PIXEL_SPACE_OFFSET_TO_PREV] || arrays_device[WPT_GT_PIXEL_SPACE_OFFSET_TO_NEXT])
            && (camera->surround_mode != WPT_SURROUND_OFF || camera->stereoscopic_distance > 0.0f))
        return fail(WPT_ERR_UNSUPPORTED, "pixel space offsets exist for Surround_Off, non-stereoscopic cameras only (camera.hpp:207-208)");
    GroundTruthArgs args;
    args.scene = scene->view;
    args.cam = *camera;
    args.camPrev = camera_prev ? *camera_prev : *camera;
    args.camNext = camera_next ? *camera_next : *camera;
    args.par = *params;
    args.t0 = times ? times[0] : 0.0f;
    args.tPrev = times ? times[1] : 0.0f;
    args.tNext = times ? times[2] : 0.0f;
    args.par.t0 = args.par.t1 = args.t0; /* one moment, no exposure interval */
    args.width = width;
    args.height = height;
    bool any = false;
    for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++) {
        args.array[k] = arrays_device[k];
        any = any || arrays_device[k];
    }
    if (!any)
        return WPT_OK;
    launchGroundTruth(args, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_ground_truth(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_host[WPT_GT_ARRAY_COUNT])
{
    if (!arrays_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    const size_t pixels = size_t(width) * height;
    void* dev[WPT_GT_ARRAY_COUNT];
    for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++)
        dev[k] = nullptr;
    wpt_status st = WPT_OK;
    for (int k = 0; k < WPT_GT_ARRAY_COUNT && st == WPT_OK; k++) {
        if (arrays_host[k] && pixels > 0) {
            hipError_t e = hipMalloc(&dev[k], pixels * wpt_gt_components[k] * 4);
            if (e != hipSuccess)
                st = fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
    }
    if (st == WPT_OK)
        st = wpt_ground_truth_device(scene, camera, camera_prev, camera_next, times, params, width, height, dev, nullptr);
    if (st == WPT_OK) {
        hipError_t e = hipDeviceSynchronize();
        for (int k = 0; k < WPT_GT_ARRAY_COUNT && e == hipSuccess; k++)
            if (dev[k])
                e = hipMemcpy(arrays_host[k], dev[k], pixels * wpt_gt_components[k] * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string("ground truth: ") + hipGetErrorString(e));
    }
    for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++)
        if (dev[k])
            (void)hipFree(dev[k]);
    return st;
}

namespace {

/* what a first-hit colour pass is refused for, before a device is needed; `out`: albedo, emission and the three guide arrays */
wpt_status firstHitCheck(const wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        void* const out[5])
{
    if (!scene || !camera || !params)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: NULL argument");
    if (width == 0 || height == 0 || width > wptdn::SIDE_MAX || height > wptdn::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: width and height must lie in 1 .. " + std::to_string(uint32_t(wptdn::SIDE_MAX)));
    const size_t pixels = size_t(width) * height;
    const size_t bytes[5] = { pixels * 12, pixels * 12, pixels * 12, pixels * 12, pixels * 4 };
    bool any = false;
    for (int k = 0; k < 5; k++) {
        any = any || out[k];
        for (int j = 0; j < k; j++) {
            const uintptr_t x = reinterpret_cast<uintptr_t>(out[k]), y = reinterpret_cast<uintptr_t>(out[j]);
            if (out[k] && out[j] && x < y + bytes[j] && y < x + bytes[k])
                return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: two outputs overlap");
        }
    }
    if (!any)
        return fail(WPT_ERR_INVALID_ARGUMENT, "first-hit colours: no output is wanted (all five arrays are NULL)");
    if (camera->surround_mode > WPT_SURROUND_360)
        return fail(WPT_ERR_UNSUPPORTED, "camera surround mode is not known to the kernel");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_UNSUPPORTED, "lens distortion model is not known to the kernel");
    return WPT_OK;
}

}

wpt_status wpt_first_hit_colours_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width,
        uint32_t height, float* albedo_device, float* emission_device, void* const guide_device[3], void* hip_stream)
{
    void* const out[5] = { albedo_device, emission_device, guide_device ? guide_device[0] : nullptr, guide_device ? guide_device[1] : nullptr,
        guide_device ? guide_device[2] : nullptr };
    WPT_TRY(firstHitCheck(scene, camera, params, width, height, out));
    wptk::FirstHitArgs args;
    args.scene = scene->view;
    args.cam = *camera;
    args.par = *params;
    args.par.t1 = args.par.t0; /* one moment, no exposure interval */
    args.width = width;
    args.height = height;
    args.albedo = albedo_device;
    args.emission = emission_device;
    args.positions = static_cast<float*>(out[2]);
    args.normals = static_cast<float*>(out[3]);
    args.materials = static_cast<int32_t*>(out[4]);
    wptk::launchFirstHitColours(args, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_first_hit_colours(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        float* albedo_host, float* emission_host, void* const guide_host[3])
{
    void* const host[5] = { albedo_host, emission_host, guide_host ? guide_host[0] : nullptr, guide_host ? guide_host[1] : nullptr,
        guide_host ? guide_host[2] : nullptr };
    WPT_TRY(firstHitCheck(scene, camera, params, width, height, host));
    const size_t pixels = size_t(width) * height;
    const size_t bytes[5] = { pixels * 12, pixels * 12, pixels * 12, pixels * 12, pixels * 4 };
    void* dev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    wpt_status st = WPT_OK;
    for (int k = 0; k < 5 && st == WPT_OK; k++) {
        if (host[k]) {
            const hipError_t e = hipMalloc(&dev[k], bytes[k]);
            if (e != hipSuccess)
                st = fail(e == hipErrorOutOfMemory ? WPT_ERR_OUT_OF_MEMORY : WPT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
    }
    if (st == WPT_OK)
        st = wpt_first_hit_colours_device(scene, camera, params, width, height, static_cast<float*>(dev[0]), static_cast<float*>(dev[1]), dev + 2,
                nullptr);
    if (st == WPT_OK) {
        hipError_t e = hipDeviceSynchronize();
        for (int k = 0; k < 5 && e == hipSuccess; k++)
            if (dev[k])
                e = hipMemcpy(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string("first-hit colours: ") + hipGetErrorString(e));
    }
    for (int k = 0; k < 5; k++)
        if (dev[k])
            (void)hipFree(dev[k]);
    return st;
}

wpt_status wpt_set_launch_config(uint32_t threads_per_group, uint32_t variant)
{
    if (threads_per_group != 0 && threads_per_group != WG)
        return fail(WPT_ERR_UNSUPPORTED, "this build uses 256 threads per workgroup");
    g_threadsPerGroup = WG;
    g_variant = variant & 0xffu;
    g_leaveEighths = 0;
    g_heavyMin = 0;
    g_leafBias = 0;
    if ((variant >> 8) & 0xffu)
        g_leaveEighths = ((variant >> 8) & 0xffu) - 1; /* byte 1: leave threshold in eighths, plus one */
    if ((variant >> 16) & 0xffu)
        g_heavyMin = ((variant >> 16) & 0xffu) - 1;     /* byte 2: lanes a long block needs, plus one */
    if ((variant >> 24) & 0xffu)
        g_leafBias = (variant >> 24) & 0xffu;           /* byte 3: leaf bias */
    return WPT_OK;
}

wpt_status wpt_set_wavefront(uint32_t mode, uint32_t groups, uint32_t chunk, uint32_t flags)
{
    if (mode > 2u)
        return fail(WPT_ERR_INVALID_ARGUMENT, "wavefront mode must be 0, 1 or 2");
    g_wfMode = mode;
    g_wfConfig.groups = groups & 0xffu;
    g_wfConfig.tracePerCu = (groups >> 8) & 0xffu; /* measurements: workgroups of the trace per compute unit */
    g_wfConfig.shadePerKind = (groups >> 16) & 1u; /* measurements: one shade launch per kind of material */
    g_wfConfig.chunk = chunk;
    g_wfConfig.buckets = (flags & 1u) ? 0u : 1u;
    g_wfConfig.refillIdle = (flags >> 8) & 0x3fu;
    g_wfConfig.leafBias = 0;
    /* bits 16-31: node steps a ray takes per launch of the trace before it is suspended (0 = default, 0xffff = no limit) */
    g_wfConfig.stepBudget = (flags >> 16) == 0xffffu ? 0xffffffffu : (flags >> 16);
    /* bits 1-7: nodes in front of the node array that the trace walks from LDS, in units of 128 (0 = default, 0x7f = none) */
    g_wfConfig.topNodes = ((flags >> 1) & 0x7fu) == 0x7fu ? 0xffffffffu : ((flags >> 1) & 0x7fu) * 128u;
    return WPT_OK;
}

wpt_status wpt_set_top_nodes(uint32_t nodes)
{
    g_topNodes = nodes & 0x7fffffffu;
    return WPT_OK;
}

wpt_status wpt_set_walk(uint32_t flags)
{
    if (flags & ~(WPT_WALK_WIDE | WPT_WALK_FULL_SHADOW | WPT_WALK_COUNT_PRODUCT | WPT_WALK_TRIANGLES_AS_GIVEN | WPT_WALK_SELECT_CORNERS | WPT_WALK_NO_FOLD | WPT_WALK_NO_BYPASS))
        return fail(WPT_ERR_INVALID_ARGUMENT, "unknown walk flag");
    g_walk = flags;
    return WPT_OK;
}

wpt_status wpt_slices_plan(uint32_t block_size, uint32_t lanes_at_once, uint32_t samples_sqrt, uint32_t* units, uint32_t* rows)
{
    if (!units || !rows)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    wptk::slicesPlan(block_size, lanes_at_once, samples_sqrt, units, rows);
    return WPT_OK;
}

wpt_status wpt_kernel_choice(uint32_t need, uint32_t sensor, uint32_t count, uint32_t node_count, uint32_t tri_count, uint32_t material_count,
        uint32_t scene_has_wide, uint32_t variant, uint32_t walk, const char** name, const char** form, uint32_t key[4],
        uint64_t* scene_lds_bytes, uint32_t* materials_in_lds)
{
    if (!name || !form || !key || !scene_lds_bytes || !materials_in_lds)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor: 0 frame, 1 transient, 2 views, 3 adaptive, 4 time of flight");
    const wptk::KernelChoice choice = wptk::selectKernel({ need, wptk::Sensor(sensor), count != 0, node_count, tri_count, material_count,
            scene_has_wide != 0, variant, walk });
    const wptk::KernelEntry* kernel = nullptr;
    const wpt_status found = lookupKernel(choice.features, choice.count, choice.ldsScene, choice.wide, &kernel);
    if (found != WPT_OK)
        return found;
    *name = kernel->name;
    *form = kernelForm(choice.rotated);
    key[0] = kernel->features;
    key[1] = kernel->count;
    key[2] = kernel->ldsScene;
    key[3] = kernel->wide;
    *scene_lds_bytes = choice.sceneLdsBytes;
    *materials_in_lds = choice.materialsInLds;
    return WPT_OK;
}

wpt_status wpt_launch_plan(uint32_t sensor, uint32_t count, uint32_t need, uint32_t scene_in_lds, uint32_t block_size, uint32_t samples_sqrt,
        uint32_t cu_count, uint32_t variant, uint32_t wavefront_mode, uint32_t slices, uint32_t plan[WPT_PLAN_WORDS])
{
    if (!plan)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor: 0 frame, 1 transient, 2 views, 3 adaptive, 4 time of flight");
    if (wavefront_mode > 2u)
        return fail(WPT_ERR_INVALID_ARGUMENT, "wavefront mode must be 0, 1 or 2");
    const wptk::LaunchPlan p = wptk::planLaunch({ sensor, count != 0, (need & FEAT_RGL) != 0, (need & FEAT_ANIM) != 0, scene_in_lds != 0,
            block_size, samples_sqrt, cu_count, variant, wavefront_mode, slices });
    const uint32_t words[WPT_PLAN_WORDS] = { p.wavefront, p.wavefrontFallBack, p.pooled, p.strategy, p.units, p.rows, p.passes };
    memcpy(plan, words, sizeof(words));
    return WPT_OK;
}

wpt_status wpt_kernel_table_entry(uint32_t index, uint32_t key[4], const char** name)
{
    if (!key || !name)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (index >= wptk::KERNEL_TABLE_ROWS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the kernel table has " + std::to_string(wptk::KERNEL_TABLE_ROWS) + " rows");
    const wptk::KernelEntry& k = wptk::KERNEL_TABLE[index];
    key[0] = k.features;
    key[1] = k.count;
    key[2] = k.ldsScene;
    key[3] = k.wide;
    *name = k.name;
    return WPT_OK;
}

wpt_status wpt_set_slices(uint32_t n)
{
    if ((n & ~WPT_SLICES_DECLINE_ODD) > wptk::SLICE_UNITS_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "slices: 0 (the library's plan), 1 (never) or 2 .. 15 units, with or without WPT_SLICES_DECLINE_ODD");
    g_slices = n;
    return WPT_OK;
}

wpt_status wpt_last_slice_stats(uint64_t* taken, uint64_t* continued)
{
    if (!taken || !continued)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *taken = 0;
    *continued = 0;
    const unsigned long long* stats = g_lastSliceStats.load(std::memory_order_relaxed);
    if (!stats)
        return WPT_OK;
    unsigned long long host[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, stats, sizeof(host), hipMemcpyDeviceToHost));
    *taken = host[0];
    *continued = host[1];
    return WPT_OK;
}

wpt_status wpt_scene_folded_links(const wpt_scene* scene, uint32_t* folded)
{
    if (!scene || !folded)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *folded = scene->foldedLinks;
    return WPT_OK;
}

wpt_status wpt_fold_plan(const wpt_scene_desc* desc, uint32_t* folded, uint32_t* lds_words)
{
    if (!folded)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(validate(desc));
    /* the device nodes of wpt_scene_upload with nothing in front (depth-first: the storage order of every tree that fits LDS)
     * and the triangles as given */
    wptl::DeviceNodes nodes;
    WPT_TRY(layoutStatus(wptl::deviceNodes(desc, wptl::triangleOrder(desc, true), 0, &nodes)));
    *folded = wptl::countFoldedLinks(reinterpret_cast<const uint32_t*>(nodes.quads.data()), desc->node_count, lds_words);
    return WPT_OK;
}

wpt_status wpt_set_bypass(uint32_t mode)
{
    if (mode > wptb::MODE_ALL_ELIGIBLE)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bypass mode: 0 (the cost model's choice) or 1 (every eligible inner node)");
    g_bypassMode = mode;
    return WPT_OK;
}

wpt_status wpt_scene_bypassed_nodes(const wpt_scene* scene, uint32_t* count)
{
    if (!scene || !count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = scene->bypassedNodes;
    return WPT_OK;
}

wpt_status wpt_bypass_plan(const wpt_scene_desc* desc, uint32_t* count, uint32_t* words)
{
    if (!count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(validate(desc));
    /* as wpt_fold_plan: the description's own depth-first order and triangle indices */
    wptl::DeviceNodes nodes;
    WPT_TRY(layoutStatus(wptl::deviceNodes(desc, wptl::triangleOrder(desc, true), 0, &nodes)));
    const uint32_t* n = reinterpret_cast<const uint32_t*>(nodes.quads.data());
    *count = 0;
    std::vector<uint32_t> links;
    if (size_t(desc->node_count) * 32 + size_t(desc->tri_count) * 48 <= LDS_SCENE_MAX_BYTES) {
        const wptb::Plan plan = wptb::plan(n, desc->node_count, desc->tri_geom, desc->tri_count, g_bypassMode);
        *count = plan.outCount;
        links = plan.bypass;
    } else { /* a tree that is not walked from LDS has no plan: the fold's links */
        links = wptb::linkWords(n, desc->node_count, true, nullptr);
    }
    if (words) {
        memcpy(words, links.data(), 2 * size_t(desc->node_count) * 4);
        words[2 * size_t(desc->node_count)] = links[2 * size_t(desc->node_count) + 2]; /* the node a ray starts at */
    }
    return WPT_OK;
}

/* Waits for the device and reports an error of any launch since the last call (a fault inside a kernel surfaces
 * here).  The kernels themselves have no bounded waits that could run out: every loop ends with its work. */
wpt_status wpt_scene_check(wpt_scene* scene)
{
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "scene is NULL");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

/* profiling hook: device buffer of 11 uint64 that counted launches add their wave-scheduler
 * statistics to (rounds, loop iterations and lane counts per state); NULL switches it off */
namespace {
static wpt_status postprocLaunch(int op, const float* in, void* out, uint64_t pixels, float a, float b, uint32_t* maxBits, void* hip_stream)
{
    if (!in || pixels == 0 || pixels > 0x7fffffffull * 256ull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad frame for post-processing");
    hipLaunchKernelGGL(wpt_postproc_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
            op, in, out, pixels, a, b, maxBits);
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}
}

wpt_status wpt_postproc_to_srgb(const float* rgb_device, uint8_t* srgb_device, uint64_t pixels, void* hip_stream)
{
    if (!srgb_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(0, rgb_device, srgb_device, pixels, 0.0f, 0.0f, nullptr, hip_stream);
}

wpt_status wpt_postproc_uniform_rational_quantization(const float* rgb_device, float* out_device, uint64_t pixels, float max_val,
        float brightness, void* hip_stream)
{
    if (!out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(1, rgb_device, out_device, pixels, max_val, brightness, nullptr, hip_stream);
}

wpt_status wpt_postproc_scale_luminance(const float* rgb_device, float* out_device, uint64_t pixels, float factor, float clamp,
        void* hip_stream)
{
    if (!out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(2, rgb_device, out_device, pixels, factor, clamp, nullptr, hip_stream);
}

wpt_status wpt_postproc_max_luminance(const float* rgb_device, uint64_t pixels, float* result_host, void* hip_stream)
{
    if (!result_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    uint32_t* bits = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&bits), sizeof(uint32_t)));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(uint32_t), stream);
    wpt_status st = e == hipSuccess ? postprocLaunch(3, rgb_device, nullptr, pixels, 0.0f, 0.0f, bits, hip_stream) : fail(WPT_ERR_HIP, hipGetErrorString(e));
    uint32_t hostBits = 0;
    if (st == WPT_OK) {
        e = hipMemcpyAsync(&hostBits, bits, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(stream);
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string("max luminance: ") + hipGetErrorString(e));
    }
    (void)hipFree(bits);
    memcpy(result_host, &hostBits, sizeof(float));
    return st;
}

wpt_status wpt_postproc_host(int op, const float* rgb_host, void* out_host, uint64_t pixels, float a, float b)
{
    if (!rgb_host || !out_host || pixels == 0 || op < 0 || op > 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad post-processing request");
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; post-processing has no CPU fallback either");
    float* dIn = nullptr;
    void* dOut = nullptr;
    const size_t inBytes = size_t(pixels) * 3 * sizeof(float);
    const size_t outBytes = op == 0 ? size_t(pixels) * 3 : (op == 3 ? 0 : inBytes);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dIn), inBytes));
    hipError_t e = hipMemcpy(dIn, rgb_host, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && outBytes > 0)
        e = hipMalloc(&dOut, outBytes);
    wpt_status st = e == hipSuccess ? WPT_OK : fail(WPT_ERR_HIP, std::string("post-processing buffers: ") + hipGetErrorString(e));
    if (st == WPT_OK) {
        if (op == 0)
            st = wpt_postproc_to_srgb(dIn, static_cast<uint8_t*>(dOut), pixels, nullptr);
        else if (op == 1)
            st = wpt_postproc_uniform_rational_quantization(dIn, static_cast<float*>(dOut), pixels, a, b, nullptr);
        else if (op == 2)
            st = wpt_postproc_scale_luminance(dIn, static_cast<float*>(dOut), pixels, a, b, nullptr);
        else
            st = wpt_postproc_max_luminance(dIn, pixels, static_cast<float*>(out_host), nullptr);
    }
    if (st == WPT_OK && outBytes > 0) {
        e = hipMemcpy(out_host, dOut, outBytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            st = fail(WPT_ERR_HIP, std::string("post-processing download: ") + hipGetErrorString(e));
    }
    (void)hipFree(dIn);
    if (dOut)
        (void)hipFree(dOut);
    return st;
}

wpt_status wpt_set_scheduler_stats(unsigned long long* stats_device)
{
    g_schedStats = stats_device;
    return WPT_OK;
}

const char* wpt_kernel_name(void)
{
    /* the kernel family of the process's most recent render call */
    const char* name = g_kernelName.load(std::memory_order_relaxed);
    return name ? name : "wpt_pathtrace";
}

const char* wpt_kernel_form(void)
{
    return g_kernelForm.load(std::memory_order_relaxed);
}

const char* wpt_device_name(int device)
{
    thread_local std::string name;
    name.clear();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        name = std::string(prop.name) + " (" + prop.gcnArchName + ", " + std::to_string(prop.multiProcessorCount) + " CUs)";
    return name.c_str();
}

uint32_t wpt_last_render_passes(void)
{
    return g_lastPasses.load(std::memory_order_relaxed);
}

const char* wpt_build_info(void)
{
#if defined(__clang_version__)
    return "hipcc / clang " __clang_version__ ", --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt "
           "-fno-gpu-flush-denormals-to-zero";
#else
    return "unknown compiler";
#endif
}

const char* wpt_last_error(void)
{
    return g_error.c_str();
}

/* test hook: evaluates one arithmetic primitive on the device for n inputs (device pointers) */
wpt_status wpt_selftest_aabb(int n, const float* boxes_device, const float* rays_device, int32_t* out_device)
{
    if (n <= 0 || !boxes_device || !rays_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_aabb_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, boxes_device, rays_device, out_device);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

/* test hooks: the triangle test in the four forms the kernels call it in, the ray's constants, the sphere test, and the closest
 * hit of a scene with its finished record (kernels above and in wpt_k_groundtruth.hip; all pointers are device pointers) */
wpt_status wpt_selftest_triangle(int form, int n, const float* cases_device, uint32_t* out_device)
{
    if (form < 0 || form > 3 || n <= 0 || !cases_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_triangle_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, form, n, cases_device, out_device);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

wpt_status wpt_selftest_rayaux(int n, const float* dirs_device, float* out_device)
{
    if (n <= 0 || !dirs_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_rayaux_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dirs_device, out_device);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

wpt_status wpt_selftest_sphere(int n, const float* spheres_device, const float* rays_device, float* out_device)
{
    if (n <= 0 || !spheres_device || !rays_device || !out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    hipLaunchKernelGGL(wpt_selftest_sphere_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, spheres_device, rays_device, out_device);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

wpt_status wpt_selftest_hits(wpt_scene* scene, int n, const float* rays8_device, float* out15_device)
{
    if (!scene || n <= 0 || !rays8_device || !out15_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    launchSelftestHits(scene->view, n, rays8_device, out15_device, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

/* the same for rays and records in host memory (a program without the HIP runtime of its own: oracle/pin_render.cpp) */
wpt_status wpt_selftest_hits_host(wpt_scene* scene, int n, const float* rays8_host, float* out15_host)
{
    if (!scene || n <= 0 || !rays8_host || !out15_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad self test arguments");
    float *rays = nullptr, *out = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&rays), size_t(n) * 8 * sizeof(float));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&out), size_t(n) * 15 * sizeof(float));
    if (e == hipSuccess)
        e = hipMemcpy(rays, rays8_host, size_t(n) * 8 * sizeof(float), hipMemcpyHostToDevice);
    wpt_status st = e == hipSuccess ? wpt_selftest_hits(scene, n, rays, out) : fail(WPT_ERR_HIP, std::string("self test: ") + hipGetErrorString(e));
    if (st == WPT_OK && (e = hipMemcpy(out15_host, out, size_t(n) * 15 * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess)
        st = fail(WPT_ERR_HIP, std::string("self test: ") + hipGetErrorString(e));
    (void)hipFree(rays);
    (void)hipFree(out);
    return st;
}

wpt_status wpt_selftest_math(int op, int n, const float* a_device, const float* b_device, float* out_device)
{
    if (n <= 0)
        return WPT_OK;
    hipLaunchKernelGGL(wpt_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, a_device, b_device, out_device);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return WPT_OK;
}

} /* extern "C" */
