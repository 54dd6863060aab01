/*
 * wpt_k_groundtruth.hip -- getGroundTruth (wurblpt.hpp:626-761): one ray through the centre of every
 * pixel, no randomness, and the geometry / material / flow buffers of its first hit.
 *
 * One lane = one pixel, one ray: the walk is the reference's BVH::hit in the stackless form the path
 * tracing kernels use, the hit record and the material tangent space are theirs too (wpt_device.h),
 * the ray comes from blockNew (wpt_blocks.h) with the pixel jitter and the lens sampling switched off.
 * The picture is taken at t0; the flow arrays compare the hit point's place at tPrev / tNext (it moves
 * with an animated instance) as seen by the camera at those times.
 */
#define WPT_SPHERE_HIT_INLINE /* see wpt_device.h: a real call would pin the kernel arguments to scratch memory */
#include "wpt_closest_hit.h" /* the walk, shared with wpt_k_firsthit.hip */

namespace wptk {

/* Camera::cameraSpaceToImageSpace (camera.hpp:194-217) */
WPT_D f2 cameraSpaceToImageSpace(const wpt_camera& cam, f3 p)
{
    const float P00 = 2.0f / (cam.r - cam.l);
    const float P11 = 2.0f / (cam.t - cam.b);
    const float P03 = (cam.r + cam.l) / (cam.r - cam.l);
    const float P13 = (cam.t + cam.b) / (cam.t - cam.b);
    const float px = P00 * p.x + P03 * p.z;
    const float py = P11 * p.y + P13 * p.z;
    const float pw = -p.z;
    f2 ic;
    ic.x = 0.5f * (px / pw) + 0.5f;
    ic.y = 0.5f * (py / pw) + 0.5f;
    wptlens::distort(cam, ic.x, ic.y);
    return ic;
}

WPT_D void store2(void* array, uint32_t pixel, f2 v)
{
    if (array) {
        float* o = static_cast<float*>(array) + 2 * (size_t)pixel;
        o[0] = v.x;
        o[1] = v.y;
    }
}
WPT_D void store1(void* array, uint32_t pixel, float v)
{
    if (array)
        static_cast<float*>(array)[pixel] = v;
}

__global__ void __launch_bounds__(256) wpt_ground_truth_kernel(const GroundTruthArgs args)
{
    const uint32_t pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= args.width * args.height)
        return;
    const SceneView& sv = args.scene;

    /* the ray: pixel centre, pinhole (getRay(..., withRandomness = false), wurblpt.hpp:660-662) */
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
    f3 wsPos = zero3, wsGNrm = zero3, wsGTan = zero3, wsMNrm = zero3, wsMTan = zero3;
    f3 csPos = zero3, csGNrm = zero3, csGTan = zero3, csMNrm = zero3, csMTan = zero3;
    float csDepth = 0.0f, csDist = 0.0f;
    f2 txCor;
    txCor.x = txCor.y = 0.0f;
    f3 wsOP = zero3, wsON = zero3, csOP = zero3, csON = zero3;
    f2 psOP = txCor, psON = txCor;
    int matInd = -1;
    if (best.prim != NO_HIT) {
        const Hit h = finishHit<GT_FEATURES>(sv, best, ps.o, ps.d, ps.time);
        wsPos = h.p;
        wsGNrm = h.n;
        wsGTan = h.t;
        /* the hitable's own material: a two-sided wrapper is not looked through (wurblpt.hpp:675) */
        const Frame ts = tangentSpaceAt<GT_FEATURES>(sv, sv.materials[h.material], h);
        wsMNrm = ts.n;
        wsMTan = ts.t;
        const InverseTransformation inv0 = inverseOf(args.cam);
        csPos = add(quatRotate(inv0.rotation, wsPos), inv0.translation);
        csGNrm = quatRotate(inv0.rotation, wsGNrm);
        csGTan = quatRotate(inv0.rotation, wsGTan);
        csMNrm = quatRotate(inv0.rotation, wsMNrm);
        csMTan = quatRotate(inv0.rotation, wsMTan);
        csDepth = -csPos.z;
        csDist = __builtin_sqrtf(dot(csPos, csPos));
        txCor = h.tc;
        f3 wsPosPrev = wsPos, wsPosNext = wsPos;
        int ai = -1;
        if (best.prim & PRIM_SPHERE) {
            ai = sv.spheres[best.prim & ~PRIM_SPHERE].animation;
        } else {
            const uint32_t inst = __float_as_uint(sv.triGeom[3 * (size_t)best.prim].w);
            if (__float_as_uint(sv.triGeom[3 * (size_t)best.prim + 2].w) & WPT_TRI_ANIMATE)
                ai = sv.instances[inst].animation;
        }
        if (ai >= 0) {
            /* wurblpt.hpp:695-699: back to where the instance keeps the point, then to where it is at tPrev / tNext */
            const wptanim::Trs T0 = animationAt(sv, ai, args.t0);
            wptanim::Trs inv;
            inv.q[0] = -T0.q[0];
            inv.q[1] = -T0.q[1];
            inv.q[2] = -T0.q[2];
            inv.q[3] = T0.q[3];
            for (int k = 0; k < 3; k++)
                inv.s[k] = 1.0f / T0.s[k];
            const f3 invT = quatRotate(inv.q, mul(neg(ld3(T0.t)), ld3(inv.s)));
            inv.t[0] = invT.x;
            inv.t[1] = invT.y;
            inv.t[2] = invT.z;
            const float pos[3] = { wsPos.x, wsPos.y, wsPos.z };
            float posOrig[3], moved[3];
            wptanim::applyTrs(inv, pos, posOrig);
            wptanim::applyTrs(animationAt(sv, ai, args.tPrev), posOrig, moved);
            wsPosPrev = mk3(moved[0], moved[1], moved[2]);
            wptanim::applyTrs(animationAt(sv, ai, args.tNext), posOrig, moved);
            wsPosNext = mk3(moved[0], moved[1], moved[2]);
        }
        wsOP = sub(wsPosPrev, wsPos);
        wsON = sub(wsPosNext, wsPos);
        const InverseTransformation invP = inverseOf(args.camPrev), invN = inverseOf(args.camNext);
        const f3 csPosPrev = add(quatRotate(invP.rotation, wsPosPrev), invP.translation);
        const f3 csPosNext = add(quatRotate(invN.rotation, wsPosNext), invN.translation);
        csOP = sub(csPosPrev, csPos);
        csON = sub(csPosNext, csPos);
        if (args.array[17] || args.array[18]) {
            const float fw = (float)args.width, fh = (float)args.height;
            f2 psPos;
            psPos.x = (((float)(pixel % args.width) + 0.5f) * (1.0f / fw)) * fw;
            psPos.y = (((float)(pixel / args.width) + 0.5f) * (1.0f / fh)) * fh;
            const f2 icPrev = cameraSpaceToImageSpace(args.cam, csPosPrev), icNext = cameraSpaceToImageSpace(args.cam, csPosNext);
            psOP.x = icPrev.x * fw - psPos.x;
            psOP.y = icPrev.y * fh - psPos.y;
            psON.x = icNext.x * fw - psPos.x;
            psON.y = icNext.y * fh - psPos.y;
        }
        matInd = (int)h.material;
    }
    store3(args.array[0], pixel, wsPos);
    store3(args.array[1], pixel, wsGNrm);
    store3(args.array[2], pixel, wsGTan);
    store3(args.array[3], pixel, wsMNrm);
    store3(args.array[4], pixel, wsMTan);
    store3(args.array[5], pixel, csPos);
    store3(args.array[6], pixel, csGNrm);
    store3(args.array[7], pixel, csGTan);
    store3(args.array[8], pixel, csMNrm);
    store3(args.array[9], pixel, csMTan);
    store1(args.array[10], pixel, csDepth);
    store1(args.array[11], pixel, csDist);
    store2(args.array[12], pixel, txCor);
    store3(args.array[13], pixel, wsOP);
    store3(args.array[14], pixel, wsON);
    store3(args.array[15], pixel, csOP);
    store3(args.array[16], pixel, csON);
    store2(args.array[17], pixel, psOP);
    store2(args.array[18], pixel, psON);
    if (args.array[19])
        static_cast<int32_t*>(args.array[19])[pixel] = matInd;
}

/* wpt_selftest_hits: BVH::hit for given rays at time 0 and the finished record, in the layout of the restatement's
 * wpt_oracle_bvh_hits: haveHit, prim, a, position, normal, tangent, texcoords, backside (all zero without a hit) */
struct SelftestHitsArgs {
    SceneView scene;
    int n;
    const float* rays8;
    float* out15;
};
__global__ void __launch_bounds__(256) wpt_selftest_hits_kernel(const SelftestHitsArgs args)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= args.n)
        return;
    const SceneView& sv = args.scene;
    const float* r = args.rays8 + 8 * (size_t)i;
    const f3 o = ld3(r), d = ld3(r + 3);
    const Candidate best = closestHit(sv, o, d, r[6], r[7], 0.0f);
    float* out = args.out15 + 15 * (size_t)i;
    for (int k = 0; k < 15; k++)
        out[k] = 0.0f;
    if (best.prim != NO_HIT) {
        const Hit h = finishHit<GT_FEATURES>(sv, best, o, d, 0.0f);
        out[0] = 1.0f;
        out[1] = (float)(best.prim & ~PRIM_SPHERE);
        out[2] = h.a;
        out[3] = h.p.x; out[4] = h.p.y; out[5] = h.p.z;
        out[6] = h.n.x; out[7] = h.n.y; out[8] = h.n.z;
        out[9] = h.t.x; out[10] = h.t.y; out[11] = h.t.z;
        out[12] = h.tc.x; out[13] = h.tc.y;
        out[14] = h.backside ? 1.0f : 0.0f;
    }
}

void launchSelftestHits(const SceneView& scene, int n, const float* rays8, float* out15, hipStream_t stream)
{
    SelftestHitsArgs args;
    args.scene = scene;
    args.n = n;
    args.rays8 = rays8;
    args.out15 = out15;
    hipLaunchKernelGGL(wpt_selftest_hits_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, args);
}

void launchGroundTruth(const GroundTruthArgs& args, hipStream_t stream)
{
    const uint32_t pixels = args.width * args.height;
    hipLaunchKernelGGL(wpt_ground_truth_kernel, dim3((pixels + 255) / 256), dim3(256), 0, stream, args);
}

}
