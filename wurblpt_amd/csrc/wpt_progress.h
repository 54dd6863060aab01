/* wpt_progress.h -- the launchers of wpt_k_progress.hip (progressive sessions, wpt_capi_progress.hip) */
#ifndef WPT_PROGRESS_H
#define WPT_PROGRESS_H

#include "wpt_pathtrace.inc.h"

namespace wptk {

/* out[3 * p + c] = inv * carry[2 * p + 1][c] for the pixels p of [blockStart, blockStart + blockSize) */
void launchProgressResolve(const float4* carry, float* out, uint32_t blockStart, uint32_t blockSize, float inv, hipStream_t stream);
/* order[at] = the pixel behind lane index `at` of the launch that `args` describes (lanePixel), *count = args.blockSize */
void launchProgressFrameOrder(const KernelArgs& args, uint32_t* order, uint32_t* count, hipStream_t stream);
/* carry[2 * p + 1] = (frame[3 * p ..], stratum) for the block's pixels: what a finished session keeps of its frame */
void launchProgressCapture(const float* frame, float4* carry, uint32_t blockStart, uint32_t blockSize, uint32_t stratum, hipStream_t stream);

}

#endif
