/* wpt_closest_hit.h -- the walk of the first-hit passes (wpt_k_groundtruth.hip, wpt_k_firsthit.hip): one ray, the closest
 * candidate.  Both passes trace the same ray with the same code, so the guide arrays of the one are the arrays of the other. */
#ifndef WPT_CLOSEST_HIT_H
#define WPT_CLOSEST_HIT_H

#include "wpt_pathtrace.inc.h"

namespace wptk {

constexpr uint32_t GT_FEATURES = FEAT_TEXTURES | FEAT_LENS | FEAT_SPHERES | FEAT_ANIM;

/* BVH::hit (bvh.hpp:270-329) in the stackless form: the closest candidate in [amin, amax], later candidates win ties */
WPT_D Candidate closestHit(const SceneView& sv, f3 o, f3 d, float amin, float amax, float time)
{
    const RayAux aux = rayAux(d);
    Candidate best;
    best.prim = NO_HIT;
    best.a = best.invDet = best.U = best.V = best.W = 0.0f;
    uint32_t node = 0;
    while (node < sv.nodeCount) {
        const float4 n0 = sv.nodes[2 * node], n1 = sv.nodes[2 * node + 1];
        const uint32_t skip = __float_as_uint(n1.z);
        const uint32_t prim = __float_as_uint(n1.w);
        const bool hit = boxTest(nodeLo(n0, n1), nodeHi(n0, n1), o, aux.inv, amin, amax);
        if (hit && prim < NODE_CHILD) {
            Candidate c;
            bool accepted;
            if (prim & PRIM_SPHERE) {
                c.invDet = c.U = c.V = c.W = 0.0f;
                accepted = sphereTest(sphereAt<GT_FEATURES>(sv, sv.spheres[prim & ~PRIM_SPHERE], time), o, d, amin, amax, c.a);
            } else {
                const float4 g0 = sv.triGeom[3 * (size_t)prim], g1 = sv.triGeom[3 * (size_t)prim + 1], g2 = sv.triGeom[3 * (size_t)prim + 2];
                f3 v0 = mk3(g0.x, g0.y, g0.z), v1 = mk3(g1.x, g1.y, g1.z), v2 = mk3(g2.x, g2.y, g2.z);
                if (__float_as_uint(g2.w) & WPT_TRI_ANIMATE) {
                    float animationM[16];
                    wptanim::toMat4(animationAt(sv, sv.instances[__float_as_uint(g0.w)].animation, time), animationM);
                    v0 = animatePoint(animationM, v0);
                    v1 = animatePoint(animationM, v1);
                    v2 = animatePoint(animationM, v2);
                }
                accepted = triangleTest(v0, v1, v2, o, aux, amin, amax, c);
            }
            if (accepted) {
                c.prim = prim;
                best = c;
                amax = c.a;
            }
            node = skip; /* a leaf's subtree is the leaf itself */
        } else {
            node = hit ? (prim & NODE_INDEX_MASK) : skip;
        }
    }
    return best;
}

/* inverse(Transformation) (transformation.hpp:157-163); applied as rotation * p + translation (wurblpt.hpp:679) */
struct InverseTransformation {
    float rotation[4];
    f3 translation;
};
WPT_D InverseTransformation inverseOf(const wpt_camera& cam)
{
    InverseTransformation inv;
    inv.rotation[0] = -cam.rotation[0];
    inv.rotation[1] = -cam.rotation[1];
    inv.rotation[2] = -cam.rotation[2];
    inv.rotation[3] = cam.rotation[3];
    const f3 invT = neg(ld3(cam.translation));
    const f3 invS = mk3(1.0f / cam.scaling[0], 1.0f / cam.scaling[1], 1.0f / cam.scaling[2]);
    inv.translation = quatRotate(inv.rotation, mul(invT, invS));
    return inv;
}

WPT_D void store3(void* array, uint32_t pixel, f3 v)
{
    if (array) {
        float* o = static_cast<float*>(array) + 3 * (size_t)pixel;
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
    }
}

}

#endif
