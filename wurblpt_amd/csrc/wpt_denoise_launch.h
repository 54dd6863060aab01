/* wpt_denoise_launch.h -- the launcher of wpt_k_denoise.hip (wpt_postproc_denoise*, wpt_capi_postproc.hip) */
#ifndef WPT_DENOISE_LAUNCH_H
#define WPT_DENOISE_LAUNCH_H

#include <hip/hip_runtime.h>

#include "wpt_denoise.h"

namespace wptk {

/* The whole filter in stream order: pack, `iterations` launches, unpack.  Every pointer is device memory; `scratch`: 4 * width *
 * height records (64 bytes per pixel), free to reuse once the stream has passed the unpack; `variance` may be NULL. */
hipError_t launchDenoise(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions, const float* normals,
        const int32_t* materials, uint32_t width, uint32_t height, const wptdn::Params& params, uint32_t iterations, wptdn::Rec* scratch,
        float* out, float* variance, hipStream_t stream);
/* The demodulated form (wpt_denoise.h, prepareDemodulated / finishDemodulated): `albedo` and `emission` are device arrays of 3
 * floats per pixel, read by the pack and again by the unpack; the iterations and the scratch are launchDenoise's. */
hipError_t launchDenoiseDemodulated(const float* frame, const float* moments, const uint16_t* samplesSqrt, const float* positions,
        const float* normals, const int32_t* materials, const float* albedo, const float* emission, uint32_t width, uint32_t height,
        const wptdn::Params& params, uint32_t iterations, float albedoFloor, wptdn::Rec* scratch, float* out, float* variance, hipStream_t stream);
/* "tile" or "gather": the form the iteration of this step takes */
const char* denoiseFormOfStep(uint32_t step);

}

#endif
