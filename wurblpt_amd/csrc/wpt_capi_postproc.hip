/*
 * wpt_capi_postproc.hip -- of include/wurblpt_hip.h: the output side, every wpt_postproc_* (sRGB, quantisation, luminance; mix,
 * mean and merge of planes; both denoisers, temporal accumulation; resample, lens warp, despeckle, distance to coordinates) and wpt_set_despeckle_form.
 * Nothing here needs the path tracer: the rules per pixel are in wpt_postproc.h, wpt_lightmix.h, wpt_denoise.h, wpt_temporal.h, wpt_image_ops.h
 * and wpt_streams.h, written once for the device and the host.  Each call's checks stand above its entry points.
 */
#include <cmath>
#include <cstring>

#define WPT_CAPI_OUTPUT_SIDE
#include "wpt_capi_common.h"
#include "wpt_math.h"
#include "wpt_postproc.h"
#include "wpt_lightmix.h"
#include "wpt_denoise_launch.h"
#include "wpt_temporal_launch.h"
#include "wpt_image_ops_launch.h"
#include "wpt_streams_launch.h"

using namespace wptc;

namespace {

struct DevicePow {
    static __device__ __forceinline__ float pow(float x, float y) { return wptm::powf_(x, y); }
};
__global__ void wpt_postproc_kernel(int op, const float* in, void* out, uint64_t pixels, float a, float b, uint32_t* maxBits)
{
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= pixels)
        return;
    wptpp::V3 rgb;
    rgb.x = in[3 * i];
    rgb.y = in[3 * i + 1];
    rgb.z = in[3 * i + 2];
    if (op == 0) {
        uint8_t* o = static_cast<uint8_t*>(out) + 3 * i;
        o[0] = wptpp::toSrgbByte<DevicePow>(rgb.x);
        o[1] = wptpp::toSrgbByte<DevicePow>(rgb.y);
        o[2] = wptpp::toSrgbByte<DevicePow>(rgb.z);
    } else if (op == 3) {
        /* maximum of non-negative floats = maximum of their bit patterns; NaN and negative values never win,
         * as in the sequential `if (y > lum)` starting from 0 */
        const float y = wptpp::luminance(rgb);
        if (y > 0.0f)
            atomicMax(maxBits, __float_as_uint(y));
    } else {
        const wptpp::V3 r = op == 1 ? wptpp::uniformRationalQuantization(rgb, a, b) : wptpp::scaleLuminance(rgb, a, b);
        float* o = static_cast<float*>(out) + 3 * i;
        o[0] = r.x;
        o[1] = r.y;
        o[2] = r.z;
    }
}

/* the mix of planes (wpt_lightmix.h): one thread per value */
__global__ void wpt_lightmix_kernel(const float* planes, uint32_t planeCount, size_t stride, uint64_t values, const float* weights, float* out)
{
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < values)
        out[i] = wptmix::mixValue(planes, planeCount, stride, weights, size_t(i));
}

} /* namespace */

extern "C" {

static wpt_status postprocLaunch(int op, const float* in, void* out, uint64_t pixels, float a, float b, uint32_t* maxBits, void* hip_stream)
{
    if (!in || pixels == 0 || pixels > 0x7fffffffull * 256ull)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad frame for post-processing");
    hipLaunchKernelGGL(wpt_postproc_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
            op, in, out, pixels, a, b, maxBits);
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_postproc_to_srgb(const float* rgb_device, uint8_t* srgb_device, uint64_t pixels, void* hip_stream)
{
    if (!srgb_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(0, rgb_device, srgb_device, pixels, 0.0f, 0.0f, nullptr, hip_stream);
}

wpt_status wpt_postproc_uniform_rational_quantization(const float* rgb_device, float* out_device, uint64_t pixels, float max_val,
        float brightness, void* hip_stream)
{
    if (!out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(1, rgb_device, out_device, pixels, max_val, brightness, nullptr, hip_stream);
}

wpt_status wpt_postproc_scale_luminance(const float* rgb_device, float* out_device, uint64_t pixels, float factor, float clamp,
        void* hip_stream)
{
    if (!out_device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    return postprocLaunch(2, rgb_device, out_device, pixels, factor, clamp, nullptr, hip_stream);
}

wpt_status wpt_postproc_max_luminance(const float* rgb_device, uint64_t pixels, float* result_host, void* hip_stream)
{
    if (!result_host)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL output");
    uint32_t* bits = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&bits), sizeof(uint32_t)));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(uint32_t), stream);
    wpt_status st = e == hipSuccess ? postprocLaunch(3, rgb_device, nullptr, pixels, 0.0f, 0.0f, bits, hip_stream) : fail(WPT_ERR_HIP, hipGetErrorString(e));
    uint32_t hostBits = 0;
    if (st == WPT_OK) {
        e = hipMemcpyAsync(&hostBits, bits, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(stream);
        st = hipStatus("max luminance", e);
    }
    (void)hipFree(bits);
    memcpy(result_host, &hostBits, sizeof(float));
    return st;
}

wpt_status wpt_postproc_host(int op, const float* rgb_host, void* out_host, uint64_t pixels, float a, float b)
{
    if (!rgb_host || !out_host || pixels == 0 || op < 0 || op > 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bad post-processing request");
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; post-processing has no CPU fallback either");
    float* dIn = nullptr;
    void* dOut = nullptr;
    const size_t inBytes = size_t(pixels) * 3 * sizeof(float);
    const size_t outBytes = op == 0 ? size_t(pixels) * 3 : (op == 3 ? 0 : inBytes);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dIn), inBytes));
    hipError_t e = hipMemcpy(dIn, rgb_host, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && outBytes > 0)
        e = hipMalloc(&dOut, outBytes);
    wpt_status st = hipStatus("post-processing buffers", e);
    if (st == WPT_OK) {
        if (op == 0)
            st = wpt_postproc_to_srgb(dIn, static_cast<uint8_t*>(dOut), pixels, nullptr);
        else if (op == 1)
            st = wpt_postproc_uniform_rational_quantization(dIn, static_cast<float*>(dOut), pixels, a, b, nullptr);
        else if (op == 2)
            st = wpt_postproc_scale_luminance(dIn, static_cast<float*>(dOut), pixels, a, b, nullptr);
        else
            st = wpt_postproc_max_luminance(dIn, pixels, static_cast<float*>(out_host), nullptr);
    }
    if (st == WPT_OK && outBytes > 0)
        st = hipStatus("post-processing download", hipMemcpy(out_host, dOut, outBytes, hipMemcpyDeviceToHost));
    (void)hipFree(dIn);
    if (dOut)
        (void)hipFree(dOut);
    return st;
}

/* what a mix is refused for, on the device or on the host */
static wpt_status mixCheck(const void* planes, uint32_t planeCount, uint64_t stride, uint64_t pixels, const void* weights, const void* out)
{
    if (!planes || !weights || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: NULL argument");
    if (planeCount == 0 || planeCount > wptmix::PLANES_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: plane count must lie in 1 .. " + std::to_string(uint32_t(wptmix::PLANES_MAX)));
    if (pixels == 0 || pixels > 0x7fffffffull * 256ull / 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: bad pixel count");
    if (planeCount > 1 && stride < pixels * 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mix of planes: the planes overlap (stride below pixels * 3)");
    return WPT_OK;
}

wpt_status wpt_postproc_mix_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_device, void* hip_stream)
{
    WPT_TRY(mixCheck(planes_device, plane_count, stride, pixels, weights_host, out_device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    StreamScratch scratch(stream);
    float* dWeights = nullptr;
    WPT_TRY(hipStatus("mix of planes", scratch.get(size_t(plane_count) * 3, &dWeights)));
    WPT_TRY(hipStatus("mix of planes", hipMemcpyAsync(dWeights, weights_host, size_t(plane_count) * 3 * sizeof(float), hipMemcpyHostToDevice, stream)));
    hipLaunchKernelGGL(wpt_lightmix_kernel, dim3(uint32_t((pixels * 3 + 255) / 256)), dim3(256), 0, stream, planes_device, plane_count,
            size_t(stride), pixels * 3, dWeights, out_device);
    return hipStatus("mix of planes", hipGetLastError());
}

wpt_status wpt_postproc_mix_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_host)
{
    WPT_TRY(mixCheck(planes_host, plane_count, stride, pixels, weights_host, out_host));
    wptmix::mixHost(planes_host, plane_count, size_t(stride), pixels, weights_host, out_host);
    return WPT_OK;
}

/* what a mean of planes is refused for, on the device or on the host */
static wpt_status meanCheck(const void* planes, uint32_t planeCount, uint64_t stride, uint64_t pixels, const void* mean)
{
    if (!planes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: the planes are NULL");
    if (!mean)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: mean_out is NULL");
    if (planeCount == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: plane_count is 0");
    if (pixels == 0 || pixels > wptk::STREAMS_MAX_VALUES / 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: bad pixel count");
    if (planeCount > 1 && stride < pixels * 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "mean of planes: the planes overlap (stride below pixels * 3)");
    return WPT_OK;
}

/* what a merge of two means is refused for, on the device or on the host */
static wpt_status mergeCheck(const void* a, uint32_t countA, const void* b, uint32_t countB, uint64_t values, const void* out)
{
    if (!a || !b || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: NULL argument");
    if (uint64_t(countA) + countB == 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: count_a + count_b is 0");
    if (values == 0 || values > wptk::STREAMS_MAX_VALUES)
        return fail(WPT_ERR_INVALID_ARGUMENT, "merge of means: bad value count");
    return WPT_OK;
}

wpt_status wpt_postproc_mean_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_device, float* moment_out_device, void* hip_stream)
{
    WPT_TRY(meanCheck(planes_device, plane_count, stride, pixels, mean_out_device));
    return hipStatus("mean of planes", wptk::launchMeanPlanes(planes_device, plane_count, size_t(stride), pixels * 3, mean_out_device, moment_out_device,
            static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_mean_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_host, float* moment_out_host)
{
    WPT_TRY(meanCheck(planes_host, plane_count, stride, pixels, mean_out_host));
    wptstr::meanHost(planes_host, plane_count, size_t(stride), pixels * 3, mean_out_host, moment_out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_merge_means(const float* a_device, uint32_t count_a, const float* b_device, uint32_t count_b, uint64_t values,
        float* out_device, void* hip_stream)
{
    WPT_TRY(mergeCheck(a_device, count_a, b_device, count_b, values, out_device));
    return hipStatus("merge of means", wptk::launchMergeMeans(a_device, count_a, b_device, count_b, values, out_device,
            static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_merge_means_host(const float* a_host, uint32_t count_a, const float* b_host, uint32_t count_b, uint64_t values,
        float* out_host)
{
    WPT_TRY(mergeCheck(a_host, count_a, b_host, count_b, values, out_host));
    wptstr::mergeHost(a_host, count_a, b_host, count_b, values, out_host);
    return WPT_OK;
}

/* the part of a denoiser call's checks that the frame's size and the parameters make up; fills in the defaults and the filter's own
 * parameters */
static wpt_status denoiseParamsCheck(uint32_t width, uint32_t height, const wpt_denoise_params* params, wptdn::Params& filter, uint32_t& iterations)
{
    if (width == 0 || height == 0 || width > wptdn::SIDE_MAX || height > wptdn::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: width and height must lie in 1 .. " + std::to_string(uint32_t(wptdn::SIDE_MAX)));
    const wpt_denoise_params defaults = { 1.0f, 0.1f, 7u, 5u };
    const wpt_denoise_params& p = params ? *params : defaults;
    if (p.iterations > WPT_DENOISE_MAX_ITERATIONS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: iterations must lie in 0 .. " + std::to_string(WPT_DENOISE_MAX_ITERATIONS));
    if (p.normal_log2 > WPT_DENOISE_MAX_NORMAL_LOG2)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: normal_log2 must lie in 0 .. " + std::to_string(WPT_DENOISE_MAX_NORMAL_LOG2));
    if (!(std::isfinite(p.sigma_l) && p.sigma_l > 0.0f) || !(std::isfinite(p.sigma_z) && p.sigma_z > 0.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: sigma_l and sigma_z must be finite and positive");
    filter.sigmaL = p.sigma_l;
    filter.sigmaZ2 = p.sigma_z * p.sigma_z;
    filter.normalLog2 = p.normal_log2;
    iterations = p.iterations;
    return WPT_OK;
}

/* what a denoiser call is refused for, on the device or on the host */
static wpt_status denoiseCheck(const void* frame, const void* moments, const void* samplesSqrt, const void* positions, const void* normals,
        const void* materials, uint32_t width, uint32_t height, const wpt_denoise_params* params, const void* out, const void* variance,
        wptdn::Params& filter, uint32_t& iterations)
{
    if (!frame || !moments || !samplesSqrt || !positions || !normals || !materials)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: an input is NULL");
    if (!out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame is NULL");
    WPT_TRY(denoiseParamsCheck(width, height, params, filter, iterations));
    /* the byte ranges of the arrays: an output may overlap neither an input nor the other output */
    const size_t pixels = size_t(width) * height;
    const struct { const void* at; size_t bytes; } in[] = { { frame, pixels * 12 }, { moments, pixels * 12 }, { samplesSqrt, pixels * 2 },
        { positions, pixels * 12 }, { normals, pixels * 12 }, { materials, pixels * 4 }, { variance, pixels * 4 } };
    for (size_t k = 0; k < sizeof(in) / sizeof(in[0]); k++) {
        if (in[k].at && overlaps(out, pixels * 12, in[k].at, in[k].bytes))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame aliases another array of the call");
        if (variance && k < 6 && overlaps(variance, pixels * 4, in[k].at, in[k].bytes))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the variance plane aliases another array of the call");
    }
    return WPT_OK;
}

/* the same for the demodulated form: the two planes of the first-hit colours beside the inputs, and the floor of the albedo */
static wpt_status denoiseDemodulatedCheck(const void* frame, const void* moments, const void* samplesSqrt, const void* positions, const void* normals,
        const void* materials, const void* albedo, const void* emission, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float& albedoFloor, const void* out, const void* variance, wptdn::Params& filter, uint32_t& iterations)
{
    if (!albedo || !emission)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the albedo or the emission plane is NULL");
    if (!std::isfinite(albedoFloor))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: albedo_floor must be finite (<= 0: the default)");
    WPT_TRY(denoiseCheck(frame, moments, samplesSqrt, positions, normals, materials, width, height, params, out, variance, filter, iterations));
    const size_t pixels = size_t(width) * height;
    for (const void* plane : { albedo, emission }) {
        if (overlaps(out, pixels * 12, plane, pixels * 12))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame aliases another array of the call");
        if (variance && overlaps(variance, pixels * 4, plane, pixels * 12))
            return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the variance plane aliases another array of the call");
    }
    if (albedoFloor <= 0.0f)
        albedoFloor = wptdn::k_albedoFloorDefault;
    return WPT_OK;
}

wpt_status wpt_postproc_denoise(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_device, float* variance_device, void* hip_stream)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseCheck(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device, materials_device, width, height,
            params, out_device, variance_device, filter, iterations));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    StreamScratch owner(stream);
    wptdn::Rec* scratch = nullptr;
    WPT_TRY(hipStatus("denoise", owner.get(size_t(width) * height * 4, &scratch)));
    return hipStatus("denoise", wptk::launchDenoise(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device,
            materials_device, width, height, filter, iterations, scratch, out_device, variance_device, stream));
}

wpt_status wpt_postproc_denoise_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_host, float* variance_host)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseCheck(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, width, height, params,
            out_host, variance_host, filter, iterations));
    std::vector<wptdn::Rec> scratch(size_t(width) * height * 4);
    wptdn::denoiseHost(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, width, height, filter,
            iterations, scratch.data(), out_host, variance_host);
    return WPT_OK;
}

const char* wpt_postproc_denoise_form(uint32_t step)
{
    return wptk::denoiseFormOfStep(step);
}

wpt_status wpt_postproc_denoise_demodulated(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, const float* albedo_device,
        const float* emission_device, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_device, float* variance_device, void* hip_stream)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseDemodulatedCheck(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device, materials_device,
            albedo_device, emission_device, width, height, params, albedo_floor, out_device, variance_device, filter, iterations));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    StreamScratch owner(stream);
    wptdn::Rec* scratch = nullptr;
    WPT_TRY(hipStatus("denoise", owner.get(size_t(width) * height * 4, &scratch)));
    return hipStatus("denoise", wptk::launchDenoiseDemodulated(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device,
            materials_device, albedo_device, emission_device, width, height, filter, iterations, albedo_floor, scratch, out_device,
            variance_device, stream));
}

wpt_status wpt_postproc_denoise_demodulated_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, const float* albedo_host,
        const float* emission_host, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_host, float* variance_host)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseDemodulatedCheck(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, albedo_host,
            emission_host, width, height, params, albedo_floor, out_host, variance_host, filter, iterations));
    std::vector<wptdn::Rec> scratch(size_t(width) * height * 4);
    wptdn::denoiseDemodulatedHost(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, albedo_host,
            emission_host, width, height, filter, iterations, albedo_floor, scratch.data(), out_host, variance_host);
    return WPT_OK;
}

/* what a call of temporal accumulation (wpt_temporal.h) is refused for, on the device or on the host; fills in the defaults and
 * the rule's own parameters */
static wpt_status temporalCheck(const void* frame, const void* moments, const void* samplesSqrt, const void* positions, const void* normals,
        const void* materials, const void* pixelOffsets, const void* cameraOffsets, const void* prev, uint32_t width, uint32_t height,
        const wpt_temporal_params* params, const void* out, const void* lengthOut, wpttm::Params& rule)
{
    if (!frame || !moments || !samplesSqrt || !positions || !normals || !materials)
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: an input is NULL");
    if (!out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: history_out is NULL");
    if (width == 0 || height == 0 || width > wptdn::SIDE_MAX || height > wptdn::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: width and height must lie in 1 .. " + std::to_string(uint32_t(wptdn::SIDE_MAX)));
    if (!pixelOffsets != !cameraOffsets)
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: the two offset arrays must both be given or both be NULL");
    const size_t pixels = size_t(width) * height, historyBytes = pixels * WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL;
    if (prev && overlaps(out, historyBytes, prev, historyBytes))
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: history_out is or overlaps history_prev (nothing works in place)");
    if (lengthOut && (overlaps(lengthOut, pixels * 4, out, historyBytes) || (prev && overlaps(lengthOut, pixels * 4, prev, historyBytes))))
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: length_out overlaps a history");
    const wpt_temporal_params defaults = { 32.0f, 0.9f, 0.02f, 0u };
    const wpt_temporal_params& p = params ? *params : defaults;
    if (!(std::isfinite(p.max_history) && p.max_history >= 1.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: max_history must be finite and at least 1");
    if (!(p.normal_cos_min >= -1.0f && p.normal_cos_min <= 1.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: normal_cos_min must lie in -1 .. 1");
    if (!(std::isfinite(p.position_tolerance) && p.position_tolerance >= 0.0f))
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: position_tolerance must be finite and not negative");
    if (p.reserved != 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "temporal accumulation: reserved must be 0");
    rule.maxHistory = p.max_history;
    rule.normalCosMin = p.normal_cos_min;
    rule.tolerance2 = p.position_tolerance * p.position_tolerance;
    return WPT_OK;
}

/* what a denoiser call on a history is refused for, on the device or on the host */
static wpt_status denoiseHistoryCheck(const void* history, uint32_t width, uint32_t height, const wpt_denoise_params* params, const void* out,
        const void* variance, wptdn::Params& filter, uint32_t& iterations)
{
    if (!history)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the history is NULL");
    if (!out)
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame is NULL");
    WPT_TRY(denoiseParamsCheck(width, height, params, filter, iterations));
    const size_t pixels = size_t(width) * height, historyBytes = pixels * WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL;
    if (overlaps(out, pixels * 12, history, historyBytes) || (variance && overlaps(out, pixels * 12, variance, pixels * 4)))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the output frame aliases another array of the call");
    if (variance && overlaps(variance, pixels * 4, history, historyBytes))
        return fail(WPT_ERR_INVALID_ARGUMENT, "denoise: the variance plane aliases another array of the call");
    return WPT_OK;
}

wpt_status wpt_postproc_temporal_accumulate(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device,
        const float* pixel_offset_to_prev_device, const float* camera_offset_to_prev_device, const void* history_prev_device,
        uint32_t width, uint32_t height, const wpt_temporal_params* params, void* history_out_device, float* length_out_device,
        void* hip_stream)
{
    wpttm::Params rule;
    WPT_TRY(temporalCheck(frame_device, moments_device, samples_sqrt_device, positions_device, normals_device, materials_device,
            pixel_offset_to_prev_device, camera_offset_to_prev_device, history_prev_device, width, height, params, history_out_device,
            length_out_device, rule));
    return hipStatus("temporal accumulation", wptk::launchTemporalAccumulate(frame_device, moments_device, samples_sqrt_device, positions_device,
            normals_device, materials_device, pixel_offset_to_prev_device, camera_offset_to_prev_device,
            static_cast<const wptdn::Rec*>(history_prev_device), width, height, rule, static_cast<wptdn::Rec*>(history_out_device),
            length_out_device, static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_temporal_accumulate_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, const float* pixel_offset_to_prev_host,
        const float* camera_offset_to_prev_host, const void* history_prev_host, uint32_t width, uint32_t height,
        const wpt_temporal_params* params, void* history_out_host, float* length_out_host)
{
    wpttm::Params rule;
    WPT_TRY(temporalCheck(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, pixel_offset_to_prev_host,
            camera_offset_to_prev_host, history_prev_host, width, height, params, history_out_host, length_out_host, rule));
    wpttm::accumulateHost(frame_host, moments_host, samples_sqrt_host, positions_host, normals_host, materials_host, pixel_offset_to_prev_host,
            camera_offset_to_prev_host, static_cast<const wptdn::Rec*>(history_prev_host), width, height, rule,
            static_cast<wptdn::Rec*>(history_out_host), length_out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_denoise_history(const void* history_device, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float* out_device, float* variance_device, void* hip_stream)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseHistoryCheck(history_device, width, height, params, out_device, variance_device, filter, iterations));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    StreamScratch owner(stream);
    wptdn::Rec* scratch = nullptr;
    if (iterations > 0)
        WPT_TRY(hipStatus("denoise", owner.get(size_t(width) * height * 2, &scratch)));
    return hipStatus("denoise", wptk::launchDenoiseHistory(static_cast<const wptdn::Rec*>(history_device), width, height, filter, iterations,
            scratch, out_device, variance_device, stream));
}

wpt_status wpt_postproc_denoise_history_host(const void* history_host, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float* out_host, float* variance_host)
{
    wptdn::Params filter;
    uint32_t iterations;
    WPT_TRY(denoiseHistoryCheck(history_host, width, height, params, out_host, variance_host, filter, iterations));
    std::vector<wptdn::Rec> scratch(iterations > 0 ? size_t(width) * height * 2 : 0);
    wpttm::denoiseHistoryHost(static_cast<const wptdn::Rec*>(history_host), width, height, filter, iterations, scratch.data(), out_host,
            variance_host);
    return WPT_OK;
}

/* what a call of the image operations (wpt_image_ops.h) is refused for, on the device or on the host: `what` names the call,
 * the output holds outWidth x outHeight x outComps floats */
static wpt_status imageOpCheck(const char* what, const void* image, uint32_t width, uint32_t height, uint32_t comps, const void* out,
        uint32_t outWidth, uint32_t outHeight, uint32_t outComps)
{
    const std::string name(what);
    if (!image || !out)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the image or the output is NULL");
    if (width == 0 || height == 0 || width > wptio::SIDE_MAX || height > wptio::SIDE_MAX || outWidth == 0 || outHeight == 0
            || outWidth > wptio::SIDE_MAX || outHeight > wptio::SIDE_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": width and height must lie in 1 .. " + std::to_string(uint32_t(wptio::SIDE_MAX)));
    if (comps < 1 || comps > wptio::COMPONENTS_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the image must have 1 .. 4 components");
    const size_t inBytes = size_t(width) * height * comps * sizeof(float), outBytes = size_t(outWidth) * outHeight * outComps * sizeof(float);
    if (overlaps(image, inBytes, out, outBytes))
        return fail(WPT_ERR_INVALID_ARGUMENT, name + ": the output overlaps the image");
    return WPT_OK;
}

/* the lens of a warp or of a distance image: only the distortion part of the camera record is read */
static wpt_status imageOpLens(const char* what, const wpt_camera* camera, wptlens::Coeffs& lens)
{
    if (!camera)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(what) + ": the camera is NULL");
    if (camera->distortion_type > WPT_DISTORTION_OPENCV)
        return fail(WPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown distortion type " + std::to_string(camera->distortion_type));
    lens = wptlens::coeffs(*camera);
    return WPT_OK;
}

static wpt_status despeckleCheck(const void* rgb, uint32_t width, uint32_t height, uint32_t comps, float minFactor, const void* out)
{
    if (rgb && out && comps != 3)
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle: the image must have 3 components");
    WPT_TRY(imageOpCheck("despeckle", rgb, width, height, 3, out, width, height, 3));
    if (!std::isfinite(minFactor))
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle: min_factor must be finite");
    return WPT_OK;
}

/* -1: as built (WPT_DESPECKLE_TILE), 0: gather, 1: tile; wpt_set_despeckle_form */
static int g_despeckleForm = -1;

static bool despeckleTile()
{
    return g_despeckleForm < 0 ? wptk::despeckleTileByDefault() : g_despeckleForm != 0;
}

wpt_status wpt_postproc_resample(const float* image_device, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_device, void* hip_stream)
{
    WPT_TRY(imageOpCheck("resample", image_device, width, height, components, out_device, new_width, new_height, components));
    const wptio::Image img = { image_device, width, height, components };
    return hipStatus("resample", wptk::launchResample(img, new_width, new_height, out_device, static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_resample_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_host)
{
    WPT_TRY(imageOpCheck("resample", image_host, width, height, components, out_host, new_width, new_height, components));
    const wptio::Image img = { image_host, width, height, components };
    wptio::resampleHost(img, new_width, new_height, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_lens_warp(const float* image_device, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_device, void* hip_stream)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("lens warp", image_device, width, height, components, out_device, width, height, components));
    WPT_TRY(imageOpLens("lens warp", camera, lens));
    const wptio::Image img = { image_device, width, height, components };
    return hipStatus("lens warp", wptk::launchLensWarp(img, lens, forward != 0, out_device, static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_lens_warp_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_host)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("lens warp", image_host, width, height, components, out_host, width, height, components));
    WPT_TRY(imageOpLens("lens warp", camera, lens));
    const wptio::Image img = { image_host, width, height, components };
    wptio::warpHost(img, lens, forward != 0, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_despeckle(const float* rgb_device, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_device, void* hip_stream)
{
    WPT_TRY(despeckleCheck(rgb_device, width, height, components, min_factor, out_device));
    return hipStatus("despeckle", wptk::launchDespeckle(rgb_device, width, height, min_factor, despeckleTile(), out_device,
            static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_despeckle_host(const float* rgb_host, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_host)
{
    WPT_TRY(despeckleCheck(rgb_host, width, height, components, min_factor, out_host));
    wptio::despeckleHost(rgb_host, width, height, min_factor, out_host);
    return WPT_OK;
}

wpt_status wpt_postproc_distance_to_coords(const float* distances_device, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_device, void* hip_stream)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("distance to coordinates", distances_device, width, height, components, coords_device, width, height, 3));
    WPT_TRY(imageOpLens("distance to coordinates", camera, lens));
    const wptio::Image img = { distances_device, width, height, components };
    return hipStatus("distance to coordinates", wptk::launchDistanceToCoords(img, lens, pmd_space != 0, coords_device,
            static_cast<hipStream_t>(hip_stream)));
}

wpt_status wpt_postproc_distance_to_coords_host(const float* distances_host, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_host)
{
    wptlens::Coeffs lens;
    WPT_TRY(imageOpCheck("distance to coordinates", distances_host, width, height, components, coords_host, width, height, 3));
    WPT_TRY(imageOpLens("distance to coordinates", camera, lens));
    const wptio::Image img = { distances_host, width, height, components };
    wptio::coordsHost(img, lens, pmd_space != 0, coords_host);
    return WPT_OK;
}

const char* wpt_postproc_despeckle_form(void)
{
    return despeckleTile() ? "tile" : "gather";
}

wpt_status wpt_set_despeckle_form(int form)
{
    if (form < -1 || form > 1)
        return fail(WPT_ERR_INVALID_ARGUMENT, "despeckle form: -1 (as built), 0 (gather) or 1 (tile)");
    g_despeckleForm = form;
    return WPT_OK;
}

void wpt_postproc_image_ops_tile(uint32_t* width, uint32_t* height)
{
    if (width)
        *width = wptk::IMAGE_OPS_TILE_W;
    if (height)
        *height = wptk::IMAGE_OPS_TILE_H;
}

} /* extern "C" */
