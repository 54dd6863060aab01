/*
 * temporal_cpp_api.cpp -- WurblPT::TemporalAccumulator (include/wurblpt/postproc.hpp) driven as an application drives it, over
 * three synthetic frames (small dyadic numbers, exact in float): a first frame, a frame at rest and a frame with motion, each
 * checked against the C host form (wpt_postproc_temporal_accumulate_host, wpt_postproc_denoise_history_host) called on the same
 * arrays; then reset().  Prints the digests of the last history, of the filtered frame and of its variance as
 * tests/denoise_check.cpp defines them, and the tag the result keeps.  Needs the library, no device.
 */
#include <cstdio>
#include <cstring>
#include <vector>

#include <wurblpt/postproc.hpp>

using namespace WurblPT;

static unsigned long long digest(const float* values, size_t count)
{
    unsigned long long sum = 0;
    for (size_t k = 0; k < count; k++) {
        uint32_t w;
        memcpy(&w, values + k, 4);
        sum += (unsigned long long)(w) * (2ull * k + 1ull);
    }
    return sum;
}

static int failures = 0;
static void check(bool good, const char* what)
{
    if (!good) {
        fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

int main()
{
    const size_t width = 20, height = 11, pixels = width * height;
    Array<float> positions(width, height, 3), normals(width, height, 3), pixelOffsets(width, height, 2), cameraOffsets(width, height, 3);
    Array<int32_t> materials(width, height, 1);
    std::vector<uint16_t> map(pixels);
    for (size_t i = 0; i < pixels; i++) {
        const size_t x = i % width, y = i / width;
        const int32_t m = int32_t((x / 4 + y / 3) % 3) - 1;
        materials[i][0] = m;
        map[i] = uint16_t(i % 4);
        for (size_t c = 0; c < 3; c++)
            normals[i][c] = (m >= 0 && c == 2) ? 1.0f : 0.0f;
        positions[i][0] = m < 0 ? 0.0f : float(x) / 32.0f;
        positions[i][1] = m < 0 ? 0.0f : float(y) / 32.0f;
        positions[i][2] = m < 0 ? 0.0f : -2.0f - 0.5f * float(m);
        /* the third frame: a quarter pixel to the left and half a pixel up, on planes that face the camera */
        pixelOffsets[i][0] = -0.25f;
        pixelOffsets[i][1] = 0.5f;
        cameraOffsets[i][0] = -0.25f / 32.0f;
        cameraOffsets[i][1] = 0.5f / 32.0f;
        cameraOffsets[i][2] = 0.0f;
    }
    TemporalParameters params;
    params.maxHistory = 2.0f;
    TemporalAccumulator accumulator(width, height, params);
    bool early = false;
    try {
        accumulator.frame();
    } catch (const std::logic_error&) {
        early = true;
    }
    check(early, "frame() before a frame throws");

    const wpt_temporal_params p = { 2.0f, 0.9f, 0.02f, 0u };
    std::vector<float> histories[2] = { std::vector<float>(pixels * 12), std::vector<float>(pixels * 12) };
    for (int k = 0; k < 3; k++) {
        Array<float> frame(width, height, 3), moments(width, height, 3);
        for (size_t i = 0; i < pixels; i++)
            for (size_t c = 0; c < 3; c++) {
                const float f = map[i] == 0 ? 0.0f : float((i * 7 + c * 3 + size_t(k) * 5) % 16) / 8.0f;
                frame[i][c] = f;
                moments[i][c] = f * f * 1.5f;
            }
        frame.globalTagList().set("WURBLPT/TEST", "kept");
        if (k < 2)
            accumulator.accumulate(frame, moments, map, positions, normals, materials);
        else
            accumulator.accumulate(frame, moments, map, positions, normals, materials, pixelOffsets, cameraOffsets);
        const bool moving = k == 2;
        check(wpt_postproc_temporal_accumulate_host(static_cast<const float*>(frame.data()), static_cast<const float*>(moments.data()), map.data(),
                    static_cast<const float*>(positions.data()), static_cast<const float*>(normals.data()),
                    static_cast<const int32_t*>(materials.data()), moving ? static_cast<const float*>(pixelOffsets.data()) : nullptr,
                    moving ? static_cast<const float*>(cameraOffsets.data()) : nullptr, k == 0 ? nullptr : histories[(k + 1) & 1].data(),
                    uint32_t(width), uint32_t(height), &p, histories[k & 1].data(), nullptr) == WPT_OK, "the C host form");
        const std::vector<float>& h = histories[k & 1];
        check(memcmp(accumulator.history(), h.data(), pixels * 48) == 0, "the history is the C host form's");
        const Array<float> f = accumulator.frame(), v = accumulator.variance(), n = accumulator.length();
        bool same = f.componentCount() == 3 && v.componentCount() == 1 && n.componentCount() == 1 && f.dimension(0) == width && f.dimension(1) == height;
        float longest = 0.0f;
        for (size_t i = 0; i < pixels && same; i++) {
            same = memcmp(&f[i][0], &h[(2 * pixels + i) * 4], 12) == 0 && memcmp(&v[i][0], &h[(2 * pixels + i) * 4 + 3], 4) == 0
                && memcmp(&n[i][0], &h[(pixels + i) * 4 + 3], 4) == 0;
            longest = n[i][0] > longest ? n[i][0] : longest;
        }
        check(same, "frame(), variance() and length() are the newest history's planes");
        check(longest == (k == 0 ? 1.0f : 2.0f), "the length grows to maxHistory and stops");
        check(f.globalTagList().value("WURBLPT/TEST") == "kept", "the frame's tags are kept");
    }
    DenoiseParameters filter;
    filter.iterations = 3;
    Array<float> variance;
    const Array<float> denoised = accumulator.denoised(filter, &variance);
    std::vector<float> out(pixels * 3), var(pixels);
    const wpt_denoise_params dp = { filter.sigmaL, filter.sigmaZ, filter.normalLog2, filter.iterations };
    check(wpt_postproc_denoise_history_host(histories[0].data(), uint32_t(width), uint32_t(height), &dp, out.data(), var.data()) == WPT_OK,
            "the C host form of the filter");
    check(memcmp(denoised.data(), out.data(), pixels * 12) == 0 && memcmp(variance.data(), var.data(), pixels * 4) == 0,
            "denoised() is the C host form's");
    printf("%016llx %016llx %016llx %s\n", digest(accumulator.history(), pixels * 12), digest(static_cast<const float*>(denoised.data()), pixels * 3),
            digest(static_cast<const float*>(variance.data()), pixels), denoised.globalTagList().value("WURBLPT/TEST").c_str());

    accumulator.reset();
    bool forgotten = false;
    try {
        accumulator.length();
    } catch (const std::logic_error&) {
        forgotten = true;
    }
    check(forgotten, "reset() forgets the history");
    bool refused = false;
    try {
        Array<float> small(3, 3, 3);
        accumulator.accumulate(small, small, map, positions, normals, materials);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    check(refused, "an array of another size is refused");
    return failures == 0 ? 0 : 1;
}
