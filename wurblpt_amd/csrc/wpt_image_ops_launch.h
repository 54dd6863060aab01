/* wpt_image_ops_launch.h -- the launchers of wpt_k_image_ops.hip (wpt_postproc_resample, _lens_warp, _despeckle and
 * _distance_to_coords, wpt_capi_postproc.hip) */
#ifndef WPT_IMAGE_OPS_LAUNCH_H
#define WPT_IMAGE_OPS_LAUNCH_H

#include <hip/hip_runtime.h>

#include "wpt_image_ops.h"

namespace wptk {

/* a workgroup's output pixels in every kernel of the unit: one lane each */
constexpr uint32_t IMAGE_OPS_TILE_W = 32, IMAGE_OPS_TILE_H = 8;

/* Every pointer is device memory; one launch each, in stream order, no scratch. */
hipError_t launchResample(const wptio::Image& img, uint32_t newWidth, uint32_t newHeight, float* out, hipStream_t stream);
hipError_t launchLensWarp(const wptio::Image& img, const wptlens::Coeffs& lens, bool forward, float* out, hipStream_t stream);
hipError_t launchDistanceToCoords(const wptio::Image& img, const wptlens::Coeffs& lens, bool pmdSpace, float* out, hipStream_t stream);
/* tile: the workgroup's pixels and their ring of neighbours go through LDS; otherwise every lane loads its nine pixels */
hipError_t launchDespeckle(const float* rgb, uint32_t width, uint32_t height, float minFactor, bool tile, float* out, hipStream_t stream);
/* the form a despeckle call takes when nothing else is asked for (WPT_DESPECKLE_TILE) */
bool despeckleTileByDefault();

}

#endif
