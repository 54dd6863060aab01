/* wpt_temporal_launch.h -- the launchers of temporal accumulation (wpt_postproc_temporal_accumulate, wpt_postproc_denoise_history;
 * wpt_capi_postproc.hip): the accumulate pass of wpt_k_temporal.hip, and the denoiser's iterations on a history, which are the
 * kernels of wpt_k_denoise.hip as they are */
#ifndef WPT_TEMPORAL_LAUNCH_H
#define WPT_TEMPORAL_LAUNCH_H

#include <hip/hip_runtime.h>

#include "wpt_temporal.h"

namespace wptk {

/* One frame into a history in stream order, one launch.  Every pointer is device memory; `pixelOffsets` and `cameraOffsets` both
 * NULL or both given; `prev` (may be NULL) and `out`: 3 * width * height records that do not overlap; `lengthOut` may be NULL.
 * Takes no scratch. */
hipError_t launchTemporalAccumulate(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions,
        const float* normals, const int32_t* materials, const float* pixelOffsets, const float* cameraOffsets, const wptdn::Rec* prev,
        uint32_t width, uint32_t height, const wpttm::Params& params, wptdn::Rec* out, float* lengthOut, hipStream_t stream);
/* The filter on a history (wpt_k_denoise.hip): `iterations` launches and the unpack.  Iteration 1 reads the history's planes,
 * later ones alternate between the two planes of `scratch` (2 * width * height records, free to reuse once the stream has passed
 * the unpack; not touched with no iterations); the history is never written.  `variance` may be NULL. */
hipError_t launchDenoiseHistory(const wptdn::Rec* history, uint32_t width, uint32_t height, const wptdn::Params& params, uint32_t iterations,
        wptdn::Rec* scratch, float* out, float* variance, hipStream_t stream);

}

#endif
