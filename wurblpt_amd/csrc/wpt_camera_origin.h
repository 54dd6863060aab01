/*
 * wpt_camera_origin.h -- the origin of a pinhole camera's rays, in a header of its own so that a host compiler can include it
 * (tests/camera_origin.cpp compares cameraOriginAtRest with the expression blockNewFrom evaluates per sample, bit for bit on the
 * CPU).  Like wpt_triangle.h, whose vector basics it uses (quatRotate among them), it compiles as device code under hipcc and
 * as plain C++ elsewhere; wpt_device.h includes it.
 */
#ifndef WPT_CAMERA_ORIGIN_H
#define WPT_CAMERA_ORIGIN_H

#include "../../include/wurblpt_hip.h"
#include "wpt_triangle.h"

namespace wptd {

/* Where the rays of a camera at rest start when they start in the camera's centre (Camera::getRay without a lens, a stereo
 * shift or a surround mode, camera.hpp:123-185): blockNewFrom's own expression with the literal zero vector in O's place.  It
 * is not the translation in general -- 0 * s is NaN for an infinite or NaN scaling and -0 for a negative one, and what the
 * rotation makes of that is added to the translation -- so nothing of it is folded: the same operations on the same operands,
 * once per launch instead of once per sample. */
WPT_D f3 cameraOriginAtRest(const wpt_camera& cam)
{
    return add(ld3(cam.translation), quatRotate(cam.rotation, mul(mk3(0.0f, 0.0f, 0.0f), ld3(cam.scaling))));
}

} /* namespace wptd */

#endif
