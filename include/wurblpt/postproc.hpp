/*
 * postproc.hpp -- the output side of a rendering: sRGB conversion and dynamic range reduction, and the image operations behind
 * them (reference interface: libwurblpt/postproc.hpp:44-337, same function names and arguments).
 *
 * toSRGB, maxLuminance, uniformRationalQuantization and scaleLuminance hand the frame to the HIP library (wpt_postproc_host in
 * wurblpt_hip.h), which runs one thread per pixel on the device; results equal the reference's loops value for value
 * (tests/test_gpu_parity.py).  There is no CPU fallback for them: without a device they throw.
 * scale, despeckle, applyLensDistortion / distort / undistort, cameraSpaceDistanceToCoords and cameraSpaceToPMDSpace call the
 * host forms of the image operations (wpt_postproc_*_host), which need no device and give the bits of the device forms and of
 * the reference's functions (tests/golden/image_ops/ holds the reference's outputs).  extractComponent(s) copy.
 */
#pragma once

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../wurblpt_hip.h"
#include "array.hpp"
#include "camera.hpp"
#include "optics.hpp"
#include "sensor.hpp"

namespace WurblPT {

namespace postprocdetail {

/* first three components of every element, tightly packed */
inline std::vector<float> packRgb(const Array<float>& img)
{
    if (img.componentCount() < 3)
        throw std::runtime_error("post-processing needs an RGB image");
    std::vector<float> rgb(img.elementCount() * 3);
    for (size_t i = 0; i < img.elementCount(); i++)
        for (size_t c = 0; c < 3; c++)
            rgb[3 * i + c] = img[i][c];
    return rgb;
}

inline void run(int op, const std::vector<float>& rgb, void* out, float a, float b)
{
    if (rgb.empty())
        return;
    if (wpt_postproc_host(op, rgb.data(), out, rgb.size() / 3, a, b) != WPT_OK)
        throw std::runtime_error(std::string("post-processing failed: ") + wpt_last_error());
}

inline Array<float> floatResult(int op, const Array<float>& img, float a, float b)
{
    const std::vector<float> rgb = packRgb(img);
    std::vector<float> out(rgb.size());
    run(op, rgb, out.data(), a, b);
    Array<float> r(img.dimension(0), img.dimension(1), img.componentCount());   /* further components stay 0 */
    r.globalTagList() = img.globalTagList();
    for (size_t i = 0; i < r.elementCount(); i++)
        for (size_t c = 0; c < 3; c++)
            r[i][c] = out[3 * i + c];
    return r;
}

}

/* Convert RGB(float) to SRGB(uint8); postproc.hpp:44-61 */
inline Array<uint8_t> toSRGB(const Array<float>& img)
{
    const std::vector<float> rgb = postprocdetail::packRgb(img);
    Array<uint8_t> r(img.dimension(0), img.dimension(1), 3);
    r.globalTagList() = img.globalTagList();
    postprocdetail::run(0, rgb, r.data(), 0.0f, 0.0f);
    return r;
}

/* postproc.hpp:65-75 */
inline float maxLuminance(const Array<float>& img)
{
    float lum = 0.0f;
    postprocdetail::run(3, postprocdetail::packRgb(img), &lum, 0.0f, 0.0f);
    return lum;
}

/* Schlick's uniform rational quantization, brightness in [1,inf); results are in [0,1] and can go
 * straight to toSRGB(); postproc.hpp:77-93 */
inline Array<float> uniformRationalQuantization(const Array<float>& img, float maxVal, float brightness)
{
    return postprocdetail::floatResult(1, img, maxVal, brightness);
}

/* postproc.hpp:95-110 */
inline Array<float> scaleLuminance(const Array<float>& img, float factor, float clamp = 1.0f)
{
    return postprocdetail::floatResult(2, img, factor, clamp);
}

/* The groups of a light-groups render weighted into one frame: an RGB weight per group sets its lamps' intensity and colour
 * after the render.  out = (((0 + w[0] * group 0) + w[1] * group 1) + ...) per channel in float (wpt_postproc_mix_planes_host in
 * wurblpt_hip.h, the same bits as the device's mix); runs on the CPU.  `weights`: groupCount() * 3 floats. */
inline Array<float> mixLightGroups(const SensorRGBLightGroups& sensor, const std::vector<float>& weights)
{
    const unsigned int K = sensor.groupCount();
    if (weights.size() != size_t(K) * 3)
        throw std::invalid_argument("mixLightGroups: an RGB weight per group (" + std::to_string(K) + " * 3 floats)");
    const size_t pixels = sensor.result().elementCount();
    std::vector<float> planes(size_t(K) * pixels * 3);
    for (unsigned int g = 0; g < K; g++) {
        const std::vector<float> rgb = postprocdetail::packRgb(sensor.group(g));
        std::copy(rgb.begin(), rgb.end(), planes.begin() + size_t(g) * pixels * 3);
    }
    Array<float> r(sensor.width(), sensor.height(), 3);
    r.globalTagList() = sensor.result().globalTagList();
    if (pixels > 0 && wpt_postproc_mix_planes_host(planes.data(), K, pixels * 3, pixels, weights.data(), static_cast<float*>(r.data())) != WPT_OK)
        throw std::runtime_error(std::string("mixLightGroups failed: ") + wpt_last_error());
    return r;
}

/* The denoiser's parameters (wpt_denoise_params in wurblpt_hip.h, which has the formula and what the defaults were measured to do) */
class DenoiseParameters
{
public:
    float sigmaL = 1.0f;          // standard deviations of luminance a tap may differ by
    float sigmaZ = 0.1f;          // sine of the angle by which a tap may leave the pixel's tangent plane
    unsigned int normalLog2 = 7;  // the normal weight is the cosine to the power 2^normalLog2
    unsigned int iterations = 5;  // a-trous iterations with steps 1, 2, 4, ...; 0 copies
};

/* A rendered frame filtered with the edge-avoiding a-trous wavelet filter under variance guidance: `frame` and `moments` are an
 * adaptive render's result and moment film (mcpt() with a sample-count map), `samplesSqrtMap` that map, and the three arrays a
 * GroundTruth's cameraSpacePositions, cameraSpaceMaterialNormals and materials at the frame's size.  Returns the filtered frame
 * with the frame's tags; `variance` (optional) receives the variance of its luminance, one component.  Runs on the CPU
 * (wpt_postproc_denoise_host, the same bits as the device's wpt_postproc_denoise). */
inline Array<float> denoise(const Array<float>& frame, const Array<float>& moments, const std::vector<uint16_t>& samplesSqrtMap,
        const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
        const DenoiseParameters& params = DenoiseParameters(), Array<float>* variance = nullptr)
{
    const size_t width = frame.dimension(0), height = frame.dimension(1), pixels = frame.elementCount();
    const Array<float>* three[3] = { &moments, &cameraSpacePositions, &cameraSpaceMaterialNormals };
    for (const Array<float>* a : three)
        if (a->elementCount() != pixels || a->dimension(0) != width || a->componentCount() != 3)
            throw std::invalid_argument("denoise: moments, positions and normals must have the frame's size and three components");
    if (materials.elementCount() != pixels || materials.dimension(0) != width || materials.componentCount() != 1 || samplesSqrtMap.size() != pixels)
        throw std::invalid_argument("denoise: the materials and the sample-count map must have the frame's size");
    const std::vector<float> rgb = postprocdetail::packRgb(frame);
    std::vector<float> out(rgb.size());
    if (variance)
        *variance = Array<float>(width, height, 1);
    const wpt_denoise_params p = { params.sigmaL, params.sigmaZ, params.normalLog2, params.iterations };
    if (wpt_postproc_denoise_host(rgb.data(), static_cast<const float*>(moments.data()), samplesSqrtMap.data(),
                static_cast<const float*>(cameraSpacePositions.data()), static_cast<const float*>(cameraSpaceMaterialNormals.data()),
                static_cast<const int32_t*>(materials.data()), uint32_t(width), uint32_t(height), &p, out.data(),
                variance ? static_cast<float*>(variance->data()) : nullptr) != WPT_OK)
        throw std::runtime_error(std::string("denoise failed: ") + wpt_last_error());
    Array<float> r(width, height, frame.componentCount());   /* further components stay 0 */
    r.globalTagList() = frame.globalTagList();
    for (size_t i = 0; i < pixels; i++)
        for (size_t c = 0; c < 3; c++)
            r[i][c] = out[3 * i + c];
    return r;
}

/* The same for a frame rendered with samplesSqrt^2 samples in every pixel */
inline Array<float> denoise(const Array<float>& frame, const Array<float>& moments, unsigned int samplesSqrt,
        const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
        const DenoiseParameters& params = DenoiseParameters(), Array<float>* variance = nullptr)
{
    if (samplesSqrt > 65535)
        throw std::invalid_argument("denoise: samplesSqrt must not exceed 65535");
    return denoise(frame, moments, std::vector<uint16_t>(frame.elementCount(), uint16_t(samplesSqrt)), cameraSpacePositions,
            cameraSpaceMaterialNormals, materials, params, variance);
}

/* The denoiser on the demodulated frame: `albedo` and `emission` (a FirstHitColours' arrays, wurblpt.hpp) are taken out of the
 * frame before the filter and put back after it, so that a texture is not filtered with the noise (wpt_postproc_denoise_
 * demodulated_host; wurblpt_hip.h has the rule).  albedoFloor <= 0: the default 1 / 64.  `variance` (optional) receives the
 * variance of the DEMODULATED luminance.  Everything else as for denoise() above. */
inline Array<float> denoise(const Array<float>& frame, const Array<float>& moments, const std::vector<uint16_t>& samplesSqrtMap,
        const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
        const Array<float>& albedo, const Array<float>& emission, const DenoiseParameters& params = DenoiseParameters(),
        float albedoFloor = 0.0f, Array<float>* variance = nullptr)
{
    const size_t width = frame.dimension(0), height = frame.dimension(1), pixels = frame.elementCount();
    const Array<float>* three[5] = { &moments, &cameraSpacePositions, &cameraSpaceMaterialNormals, &albedo, &emission };
    for (const Array<float>* a : three)
        if (a->elementCount() != pixels || a->dimension(0) != width || a->componentCount() != 3)
            throw std::invalid_argument("denoise: moments, positions, normals, albedo and emission must have the frame's size and three components");
    if (materials.elementCount() != pixels || materials.dimension(0) != width || materials.componentCount() != 1 || samplesSqrtMap.size() != pixels)
        throw std::invalid_argument("denoise: the materials and the sample-count map must have the frame's size");
    const std::vector<float> rgb = postprocdetail::packRgb(frame);
    std::vector<float> out(rgb.size());
    if (variance)
        *variance = Array<float>(width, height, 1);
    const wpt_denoise_params p = { params.sigmaL, params.sigmaZ, params.normalLog2, params.iterations };
    if (wpt_postproc_denoise_demodulated_host(rgb.data(), static_cast<const float*>(moments.data()), samplesSqrtMap.data(),
                static_cast<const float*>(cameraSpacePositions.data()), static_cast<const float*>(cameraSpaceMaterialNormals.data()),
                static_cast<const int32_t*>(materials.data()), static_cast<const float*>(albedo.data()),
                static_cast<const float*>(emission.data()), uint32_t(width), uint32_t(height), &p, albedoFloor, out.data(),
                variance ? static_cast<float*>(variance->data()) : nullptr) != WPT_OK)
        throw std::runtime_error(std::string("denoise failed: ") + wpt_last_error());
    Array<float> r(width, height, frame.componentCount());   /* further components stay 0 */
    r.globalTagList() = frame.globalTagList();
    for (size_t i = 0; i < pixels; i++)
        for (size_t c = 0; c < 3; c++)
            r[i][c] = out[3 * i + c];
    return r;
}

/* The same for a frame rendered with samplesSqrt^2 samples in every pixel */
inline Array<float> denoise(const Array<float>& frame, const Array<float>& moments, unsigned int samplesSqrt,
        const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
        const Array<float>& albedo, const Array<float>& emission, const DenoiseParameters& params = DenoiseParameters(),
        float albedoFloor = 0.0f, Array<float>* variance = nullptr)
{
    if (samplesSqrt > 65535)
        throw std::invalid_argument("denoise: samplesSqrt must not exceed 65535");
    return denoise(frame, moments, std::vector<uint16_t>(frame.elementCount(), uint16_t(samplesSqrt)), cameraSpacePositions,
            cameraSpaceMaterialNormals, materials, albedo, emission, params, albedoFloor, variance);
}

/* The parameters of temporal accumulation (wpt_temporal_params in wurblpt_hip.h, which has the rule) */
class TemporalParameters
{
public:
    float maxHistory = 32.0f;         // longest history length, in frames
    float normalCosMin = 0.9f;        // smallest accepted cosine between the current and the reprojected normal
    float positionTolerance = 0.02f;  // relative to the distance from the previous camera
};

/* Temporal accumulation in front of the denoiser: a pixel's estimate is carried from frame to frame, so that in regions that stay
 * visible F frames of n samples count as F * n samples (wpt_postproc_temporal_accumulate_host; wurblpt_hip.h has the rule and
 * the layout of a history).  Owns the two histories it alternates between (96 bytes per pixel).  Every frame of the sequence
 * must be rendered with its own samples, and all arrays have the accumulator's size.  Runs on the CPU, with the bits of the
 * device's form. */
class TemporalAccumulator
{
private:
    size_t _width, _height;
    TemporalParameters _params;
    std::vector<float> _histories[2];
    unsigned int _newest;   // index of the newest history
    bool _filled;           // false until the first frame came in, and after reset()
    TagList _tags;

    const float* newest(const char* what) const
    {
        if (!_filled)
            throw std::logic_error(std::string("TemporalAccumulator::") + what + ": no frame was accumulated yet");
        return _histories[_newest].data();
    }

    Array<float> plane(const char* what, size_t planeIndex, size_t first, size_t comps) const
    {
        const float* h = newest(what) + planeIndex * _width * _height * 4;
        Array<float> r(_width, _height, comps);
        r.globalTagList() = _tags;
        for (size_t i = 0; i < _width * _height; i++)
            for (size_t c = 0; c < comps; c++)
                r[i][c] = h[4 * i + first + c];
        return r;
    }

    void run(const Array<float>& frame, const Array<float>& moments, const std::vector<uint16_t>& samplesSqrtMap,
            const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
            const Array<float>* pixelSpaceOffsetToPrev, const Array<float>* cameraSpaceOffsetToPrev)
    {
        const size_t pixels = _width * _height;
        if (frame.elementCount() != pixels || frame.dimension(0) != _width || frame.componentCount() < 3)
            throw std::invalid_argument("TemporalAccumulator: the frame must have the accumulator's size and at least three components");
        const struct { const Array<float>* a; size_t comps; } sized[5] = { { &moments, 3 }, { &cameraSpacePositions, 3 },
            { &cameraSpaceMaterialNormals, 3 }, { pixelSpaceOffsetToPrev, 2 }, { cameraSpaceOffsetToPrev, 3 } };
        for (const auto& s : sized)
            if (s.a && (s.a->elementCount() != pixels || s.a->dimension(0) != _width || s.a->componentCount() != s.comps))
                throw std::invalid_argument("TemporalAccumulator: every array must have the accumulator's size; moments, positions and "
                        "normals three components, the pixel offsets two, the camera offsets three");
        if (materials.elementCount() != pixels || materials.dimension(0) != _width || materials.componentCount() != 1 || samplesSqrtMap.size() != pixels)
            throw std::invalid_argument("TemporalAccumulator: the materials and the sample-count map must have the accumulator's size");
        const std::vector<float> rgb = postprocdetail::packRgb(frame);
        const unsigned int target = _filled ? 1u - _newest : 0u;
        const wpt_temporal_params p = { _params.maxHistory, _params.normalCosMin, _params.positionTolerance, 0u };
        if (wpt_postproc_temporal_accumulate_host(rgb.data(), static_cast<const float*>(moments.data()), samplesSqrtMap.data(),
                    static_cast<const float*>(cameraSpacePositions.data()), static_cast<const float*>(cameraSpaceMaterialNormals.data()),
                    static_cast<const int32_t*>(materials.data()),
                    pixelSpaceOffsetToPrev ? static_cast<const float*>(pixelSpaceOffsetToPrev->data()) : nullptr,
                    cameraSpaceOffsetToPrev ? static_cast<const float*>(cameraSpaceOffsetToPrev->data()) : nullptr,
                    _filled ? _histories[_newest].data() : nullptr, uint32_t(_width), uint32_t(_height), &p, _histories[target].data(),
                    nullptr) != WPT_OK)
            throw std::runtime_error(std::string("temporal accumulation failed: ") + wpt_last_error());
        _newest = target;
        _filled = true;
        _tags = frame.globalTagList();
    }

public:
    TemporalAccumulator(size_t width, size_t height, const TemporalParameters& params = TemporalParameters()) :
        _width(width), _height(height), _params(params), _newest(0), _filled(false)
    {
        if (width == 0 || height == 0 || width > 65535 || height > 65535)
            throw std::invalid_argument("TemporalAccumulator: width and height must lie in 1 .. 65535");
        for (std::vector<float>& h : _histories)
            h.resize(width * height * (WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL / sizeof(float)));
    }

    size_t width() const { return _width; }
    size_t height() const { return _height; }

    /* the next frame of a scene and a camera at rest: an adaptive or split render's result and moment film, its sample-count map,
     * and a GroundTruth's cameraSpacePositions, cameraSpaceMaterialNormals and materials */
    void accumulate(const Array<float>& frame, const Array<float>& moments, const std::vector<uint16_t>& samplesSqrtMap,
            const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials)
    {
        run(frame, moments, samplesSqrtMap, cameraSpacePositions, cameraSpaceMaterialNormals, materials, nullptr, nullptr);
    }

    /* the next frame with motion: a GroundTruth's pixelSpaceOffsetToPrev and cameraSpaceOffsetToPrev beside the above */
    void accumulate(const Array<float>& frame, const Array<float>& moments, const std::vector<uint16_t>& samplesSqrtMap,
            const Array<float>& cameraSpacePositions, const Array<float>& cameraSpaceMaterialNormals, const Array<int32_t>& materials,
            const Array<float>& pixelSpaceOffsetToPrev, const Array<float>& cameraSpaceOffsetToPrev)
    {
        run(frame, moments, samplesSqrtMap, cameraSpacePositions, cameraSpaceMaterialNormals, materials, &pixelSpaceOffsetToPrev,
                &cameraSpaceOffsetToPrev);
    }

    /* of the newest history: the accumulated frame (three components, the last frame's tags), the variance of its luminance and
     * the history length per pixel (one component each) */
    Array<float> frame() const { return plane("frame", 2, 0, 3); }
    Array<float> variance() const { return plane("variance", 2, 3, 1); }
    Array<float> length() const { return plane("length", 1, 3, 1); }

    /* the newest history's records, [3][height][width][4] floats (wurblpt_hip.h has the layout) */
    const float* history() const { return newest("history"); }

    /* the newest history filtered by the denoiser's iterations (wpt_postproc_denoise_history_host); `variance` (optional)
     * receives the variance of the result's luminance */
    Array<float> denoised(const DenoiseParameters& params = DenoiseParameters(), Array<float>* variance = nullptr) const
    {
        const float* h = newest("denoised");
        Array<float> r(_width, _height, 3);
        r.globalTagList() = _tags;
        if (variance)
            *variance = Array<float>(_width, _height, 1);
        const wpt_denoise_params p = { params.sigmaL, params.sigmaZ, params.normalLog2, params.iterations };
        if (wpt_postproc_denoise_history_host(h, uint32_t(_width), uint32_t(_height), &p, static_cast<float*>(r.data()),
                    variance ? static_cast<float*>(variance->data()) : nullptr) != WPT_OK)
            throw std::runtime_error(std::string("denoise failed: ") + wpt_last_error());
        return r;
    }

    /* forget the history: the next frame is a first frame (a cut, a camera jump) */
    void reset() { _filled = false; }
};

/* ---- image operations (postproc.hpp:112-337) ---- */

namespace postprocdetail {

/* a float image of at most four components, or an exception */
inline void checkImage(const Array<float>& img, const char* what)
{
    if (img.elementCount() == 0 || img.componentCount() < 1 || img.componentCount() > 4)
        throw std::invalid_argument(std::string(what) + ": the image must be a float array with 1 to 4 components");
}

inline void check(wpt_status status, const char* what)
{
    if (status != WPT_OK)
        throw std::runtime_error(std::string(what) + " failed: " + wpt_last_error());
}

/* the camera record of a lens on a projection: the image operations read its distortion part only */
inline wpt_camera lensRecord(const LensDistortion& distortion, const Projection& projection)
{
    wpt_camera record = {};
    Camera(Optics(projection, distortion)).describe(record);
    return record;
}

}

/* Bilinear resampling to newWidth x newHeight; postproc.hpp:112-136 */
inline Array<float> scale(const Array<float>& img, unsigned int newWidth, unsigned int newHeight)
{
    postprocdetail::checkImage(img, "scale");
    Array<float> scaledImg({ newWidth, newHeight }, img.componentCount());
    scaledImg.globalTagList() = img.globalTagList();
    postprocdetail::check(wpt_postproc_resample_host(static_cast<const float*>(img.data()), uint32_t(img.dimension(0)), uint32_t(img.dimension(1)),
                uint32_t(img.componentCount()), newWidth, newHeight, static_cast<float*>(scaledImg.data())), "scale");
    return scaledImg;
}

/* Selective despeckling: every pixel whose luminance is the greatest of its 3x3 neighbourhood and at least minFactor times the
 * second greatest is replaced by the neighbourhood's median pixel.  Input and output are RGB images; postproc.hpp:143-193 */
inline Array<float> despeckle(const Array<float>& img, float minFactor = 1.25f)
{
    postprocdetail::checkImage(img, "despeckle");
    Array<float> out({ img.dimension(0), img.dimension(1) }, img.componentCount());
    out.globalTagList() = img.globalTagList();
    postprocdetail::check(wpt_postproc_despeckle_host(static_cast<const float*>(img.data()), uint32_t(img.dimension(0)), uint32_t(img.dimension(1)),
                uint32_t(img.componentCount()), minFactor, static_cast<float*>(out.data())), "despeckle");
    return out;
}

/* Lens distortion; postproc.hpp:197-248.  forward: true distorts the input, false undistorts it */
inline Array<float> applyLensDistortion(const Array<float>& input, const LensDistortion& distortion, const Projection& projection, bool forward)
{
    postprocdetail::checkImage(input, "applyLensDistortion");
    Array<float> output(input.dimensions(), input.componentCount());
    output.globalTagList() = input.globalTagList();
    const wpt_camera record = postprocdetail::lensRecord(distortion, projection);
    postprocdetail::check(wpt_postproc_lens_warp_host(static_cast<const float*>(input.data()), uint32_t(input.dimension(0)),
                uint32_t(input.dimension(1)), uint32_t(input.componentCount()), &record, forward ? 1 : 0, static_cast<float*>(output.data())),
            "applyLensDistortion");
    return output;
}

inline Array<float> distort(const Array<float>& undistorted, const LensDistortion& distortion, const Projection& projection)
{
    return applyLensDistortion(undistorted, distortion, projection, true);
}

inline Array<float> undistort(const Array<float>& distorted, const LensDistortion& distortion, const Projection& projection)
{
    return applyLensDistortion(distorted, distortion, projection, false);
}

/* Distance measurements (typically ToF; the first component holds the distance) to camera space coordinates; postproc.hpp:252-287 */
inline Array<float> cameraSpaceDistanceToCoords(const Array<float>& distances, const Projection& projection, const LensDistortion& distortion)
{
    postprocdetail::checkImage(distances, "cameraSpaceDistanceToCoords");
    Array<float> coords(distances.dimensions(), 3);
    coords.globalTagList() = distances.globalTagList();
    const wpt_camera record = postprocdetail::lensRecord(distortion, projection);
    postprocdetail::check(wpt_postproc_distance_to_coords_host(static_cast<const float*>(distances.data()), uint32_t(distances.dimension(0)),
                uint32_t(distances.dimension(1)), uint32_t(distances.componentCount()), &record, 0, static_cast<float*>(coords.data())),
            "cameraSpaceDistanceToCoords");
    return coords;
}

/* Camera space coordinates (the first three components are x, y, z) in the PMD camera's system; postproc.hpp:289-309 */
inline Array<float> cameraSpaceToPMDSpace(const Array<float>& coords)
{
    if (coords.componentCount() < 3)
        throw std::invalid_argument("cameraSpaceToPMDSpace: the first three components must be x, y, z");
    Array<float> pmdspace(coords.dimensions(), 3);
    pmdspace.globalTagList() = coords.globalTagList();
    for (size_t e = 0; e < pmdspace.elementCount(); e++) {
        pmdspace[e][0] = coords[e][0];
        pmdspace[e][1] = -coords[e][1];
        pmdspace[e][2] = -coords[e][2];
    }
    return pmdspace;
}

/* Components of an array, in the order of the list; postproc.hpp:313-337 */
inline ArrayContainer extractComponents(const ArrayContainer& a, const std::vector<size_t>& componentList)
{
    for (size_t component : componentList)
        if (component >= a.componentCount())
            throw std::invalid_argument("extractComponents: the array has no component " + std::to_string(component));
    ArrayContainer r(a.dimensions(), componentList.size(), a.componentType());
    r.globalTagList() = a.globalTagList();
    unsigned char* dst = static_cast<unsigned char*>(r.data());
    const unsigned char* src = static_cast<const unsigned char*>(a.data());
    for (size_t e = 0; e < a.elementCount(); e++)
        for (size_t c = 0; c < componentList.size(); c++)
            std::memcpy(dst + e * r.elementSize() + c * r.componentSize(), src + e * a.elementSize() + componentList[c] * a.componentSize(),
                    a.componentSize());
    return r;
}

inline ArrayContainer extractComponent(const ArrayContainer& a, size_t component)
{
    return extractComponents(a, { component });
}

}
