/* wpt_k_adaptive_cost.hip -- the measure an adaptive launch orders its pixels by: n_p^2 samples (wpt_k_order.hip builds the
 * order from it, longest first).  n_p <= 65535, so n_p^2 fits 32 bits. */
#include "wpt_pathtrace.inc.h"

namespace wptk {

namespace {

__global__ __launch_bounds__(256) void adaptiveCost(const KernelArgs args)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    uint32_t pixel;
    if (lanePixel(args, gid, pixel)) {
        const uint32_t n = args.adaptive.samplesSqrt[pixel];
        args.cost[pixel] = n * n;
    }
}

}

void launchAdaptiveCost(const KernelArgs& args, hipStream_t stream)
{
    hipLaunchKernelGGL(adaptiveCost, dim3((args.blockSize + 255u) / 256u), dim3(256), 0, stream, args);
}

}
