/*
 * denoise_demodulated_cpp_api.cpp -- the overload of WurblPT::denoise that takes albedo and emission (include/wurblpt/
 * postproc.hpp) called as an application calls it, on arrays whose values tests/test_denoise_demodulated_host.py makes again in
 * numpy (small dyadic numbers, exact in float): prints the digests of the filtered frame and of the variance plane for the map
 * form, then of the frame for the form with one sample count and a floor of its own, as tests/denoise_check.cpp defines them,
 * and the tag the result keeps.  Needs the library, no device.
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

int main()
{
    const size_t width = 20, height = 11;
    Array<float> frame(width, height, 3), moments(width, height, 3), positions(width, height, 3), normals(width, height, 3);
    Array<float> albedo(width, height, 3), emission(width, height, 3);
    Array<int32_t> materials(width, height, 1);
    std::vector<uint16_t> map(width * height);
    for (size_t i = 0; i < width * height; i++) {
        const size_t x = i % width, y = i / width;
        const int32_t m = int32_t((x / 4 + y / 3) % 3) - 1;
        materials[i][0] = m;
        map[i] = uint16_t(1 + i % 4);
        for (size_t c = 0; c < 3; c++) {
            const float f = float((i * 7 + c * 3) % 16) / 8.0f;
            frame[i][c] = f;
            moments[i][c] = f * f * 1.5f;
            normals[i][c] = (m >= 0 && c == 2) ? 1.0f : 0.0f;
            albedo[i][c] = float((i * 5 + c * 11) % 9) / 8.0f;       /* 0 .. 1 in eighths: 0 lies below either floor, 1/8 below the second */
            emission[i][c] = (i % 10 == 3) ? f * 0.5f : 0.0f;
        }
        positions[i][0] = m < 0 ? 0.0f : float(x) / 32.0f;
        positions[i][1] = m < 0 ? 0.0f : float(y) / 32.0f;
        positions[i][2] = m < 0 ? 0.0f : -2.0f - 0.5f * float(m);
    }
    frame.globalTagList().set("WURBLPT/TEST", "kept");
    DenoiseParameters params;
    params.iterations = 3;
    Array<float> variance;
    const Array<float> a = denoise(frame, moments, map, positions, normals, materials, albedo, emission, params, 0.0f, &variance);
    const Array<float> b = denoise(frame, moments, 2u, positions, normals, materials, albedo, emission, DenoiseParameters(), 0.25f);
    printf("%016llx %016llx %016llx %s\n", digest(static_cast<const float*>(a.data()), width * height * 3),
            digest(static_cast<const float*>(variance.data()), width * height), digest(static_cast<const float*>(b.data()), width * height * 3),
            a.globalTagList().value("WURBLPT/TEST").c_str());
    bool refused = false;
    try {
        denoise(frame, moments, map, positions, normals, materials, albedo, Array<float>(width, height, 1));
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    return refused ? 0 : 1;
}
