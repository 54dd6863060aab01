/*
 * wpt_k_firsthit.hip -- the first-hit colour pass (wpt_first_hit_colours*): what the surface a pixel's centre sees multiplies
 * the light with (albedo) and what it sends out itself (emission), for the denoiser to take out of the frame before it filters
 * and to put back afterwards (wpt_denoise.h, prepareDemodulated / finishDemodulated).
 *
 * One lane = one pixel, the ray and the walk of wpt_k_groundtruth.hip (wpt_closest_hit.h): pixel centre, pinhole, time t0.
 * The three guide arrays of the denoiser come out of the same walk, computed as the ground truth kernel computes them, so a
 * denoise needs one walk per pixel.  DESIGN.md, "Denoiser", holds the rule and its table of materials.
 */
#define WPT_SPHERE_HIT_INLINE /* see wpt_device.h: a real call would pin the kernel arguments to scratch memory */
#include "wpt_closest_hit.h"
#include "wpt_firsthit_launch.h"

namespace wptk {

/* every feature the rule can meet; the bits finishHit and tangentSpaceAt look at are those of GT_FEATURES */
constexpr uint32_t FH_FEATURES = GT_FEATURES | FEAT_MODPHONG | FEAT_ENVMAP | FEAT_TWOSIDED | FEAT_GGX | FEAT_GLASS | FEAT_SPOT;

__global__ void __launch_bounds__(256) wpt_first_hit_colours_kernel(const FirstHitArgs args)
{
    const uint32_t pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= args.width * args.height)
        return;
    const SceneView& sv = args.scene;

    /* the ray: pixel centre, pinhole, as wpt_ground_truth_kernel sets it up */
    FrameArgs fa;
    fa.cam = args.cam;
    fa.cam.lens_radius = 0.0f;
    fa.par = args.par;
    fa.par.randomize_ray_over_pixel = 0;
    fa.width = args.width;
    fa.height = args.height;
    fa.samplesSqrt = 1;
    fa.invWidth = 1.0f / (float)args.width;
    fa.invHeight = 1.0f / (float)args.height;
    fa.invSamplesSqrt = 1.0f;
    PathRegs ps;
    pathStateInit(ps, pixel, pixel % args.width, pixel / args.width);
    blockNew<GT_FEATURES>(fa, ps, sv); /* par.t0 == par.t1: no time draw, ps.time = t0 */

    const Candidate best = closestHit(sv, ps.o, ps.d, args.par.min_hit_distance, k_maxval, ps.time);

    const f3 zero3 = mk3(0.0f, 0.0f, 0.0f);
    f3 albedo = zero3, emission = zero3, csPos = zero3, csMNrm = zero3;
    int matInd = -1;
    if (best.prim != NO_HIT) {
        Hit h = finishHit<GT_FEATURES>(sv, best, ps.o, ps.d, ps.time);
        if (args.positions || args.normals) {
            /* the hitable's own material: a two-sided wrapper is not looked through (wpt_k_groundtruth.hip) */
            const Frame ts = tangentSpaceAt<GT_FEATURES>(sv, sv.materials[h.material], h);
            const InverseTransformation inv0 = inverseOf(args.cam);
            csPos = add(quatRotate(inv0.rotation, h.p), inv0.translation);
            csMNrm = quatRotate(inv0.rotation, ts.n);
        }
        matInd = (int)h.material;
        /* the colours look through it, as the path tracer does: the back child sees the hit from its front */
        const wpt_material& m = resolveMaterial<FH_FEATURES>(sv, h.material, h);
        const f4 e = materialEmitted<FH_FEATURES>(sv, m, h, ps.d);
        emission = mk3(e.x, e.y, e.z);
        switch (m.type) {
        case WPT_MAT_LAMBERTIAN:
        case WPT_MAT_GGX:
        case WPT_MAT_MIRROR:
        case WPT_MAT_MODPHONG:
            if (!h.backside) {
                const f4 a = texOrConst<FH_FEATURES>(sv, m.tex[0], m.v[0], h.tc);
                albedo = mk3(a.x, a.y, a.z);
            }
            break;
        case WPT_MAT_GLASS:
            albedo = mk3(1.0f, 1.0f, 1.0f);
            break;
        case WPT_MAT_RGL:
            if (!h.backside)
                albedo = mk3(1.0f, 1.0f, 1.0f);
            break;
        default: /* NONE, the lights */
            break;
        }
    } else if (sv.envType != WPT_ENV_NONE) {
        const f4 e = envL(sv, ps.d);
        emission = mk3(e.x, e.y, e.z);
    }
    store3(args.albedo, pixel, albedo);
    store3(args.emission, pixel, emission);
    store3(args.positions, pixel, csPos);
    store3(args.normals, pixel, csMNrm);
    if (args.materials)
        args.materials[pixel] = matInd;
}

void launchFirstHitColours(const FirstHitArgs& args, hipStream_t stream)
{
    const uint32_t pixels = args.width * args.height;
    hipLaunchKernelGGL(wpt_first_hit_colours_kernel, dim3((pixels + 255) / 256), dim3(256), 0, stream, args);
}

}
