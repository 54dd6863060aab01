/* wpt_firsthit_launch.h -- the launcher of wpt_k_firsthit.hip (wpt_first_hit_colours*, wpt_capi_first_hit.hip) */
#ifndef WPT_FIRSTHIT_LAUNCH_H
#define WPT_FIRSTHIT_LAUNCH_H

#include "wpt_pathtrace.inc.h"

namespace wptk {

/* The first-hit colour pass: every array is device memory of width * height elements of its kind, or NULL.  `par.t0 == par.t1`
 * is the moment of the picture. */
struct FirstHitArgs {
    SceneView scene;
    wpt_camera cam;
    wpt_params par;
    uint32_t width, height;
    float* albedo;      /* 3 floats per pixel */
    float* emission;    /* 3 */
    float* positions;   /* 3: WPT_GT_CAMERA_SPACE_POSITIONS */
    float* normals;     /* 3: WPT_GT_CAMERA_SPACE_MATERIAL_NORMALS */
    int32_t* materials; /* 1: WPT_GT_MATERIALS */
};
void launchFirstHitColours(const FirstHitArgs& args, hipStream_t stream);

}

#endif
