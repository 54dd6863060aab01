/*
 * denoise_check.cpp -- wurblpt_amd/csrc/wpt_denoise.h on its own: compiled outside the library, without a header of HIP, with
 * -fsanitize=address,undefined, and run as a program (tests/test_denoise_host.py).  Every buffer has exactly the size the
 * interface promises to stay within, so a read or write past it stops the program.
 *   frames (width x height) 1x1, 1x7, 5x3, 33x9, 130x70, each with every iteration count 0 .. 8, so that whole rings of taps
 *   fall outside the frame, and each in three kinds: "mixed" (several materials, sky, n_p in {0, 1, 2, 5}), "sky" (nothing
 *   hit anywhere) and "unsampled" (n_p = 0 everywhere, the frame and the moments zero)
 * Checked here: every output is finite, no variance is negative, zero iterations return the frame's own bits.
 * usage: denoise_check [DIRECTORY]
 * Prints one JSON object: "<kind>_<width>x<height>_i<iterations>" -> [digest of the frame, digest of the variance plane], a
 * digest being the sum over the 32-bit words w_k of w_k * (2 k + 1) modulo 2^64 in hexadecimal (tests/golden/denoise_digests.json
 * holds these lines; the library's host entry must reproduce them).  With a DIRECTORY, the inputs of every frame are left
 * there as <kind>_<width>x<height>.bin: frame, moments, positions, normals (3 floats per pixel each), materials (int32),
 * sample-count map (uint16).
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_denoise.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t next()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(state >> 32);
}
static float unit() { return float(next() >> 8) * (1.0f / 16777216.0f); }

static uint64_t digest(const float* values, size_t count)
{
    uint64_t sum = 0;
    for (size_t k = 0; k < count; k++) {
        uint32_t w;
        memcpy(&w, values + k, 4);
        sum += uint64_t(w) * (2 * uint64_t(k) + 1);
    }
    return sum;
}

struct Inputs {
    std::vector<float> frame, moments, positions, normals;
    std::vector<int32_t> materials;
    std::vector<uint16_t> map;
};

/* kind 0: mixed, 1: sky, 2: unsampled */
static Inputs make(uint32_t width, uint32_t height, int kind)
{
    const size_t pixels = size_t(width) * height;
    Inputs in;
    in.frame.resize(pixels * 3);
    in.moments.resize(pixels * 3);
    in.positions.resize(pixels * 3);
    in.normals.resize(pixels * 3);
    in.materials.resize(pixels);
    in.map.resize(pixels);
    static const uint16_t counts[4] = { 0, 1, 2, 5 };
    for (size_t p = 0; p < pixels; p++) {
        const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
        /* materials in patches of a few pixels, a tenth of them sky */
        int32_t m = int32_t(((x / 3) * 7 + (y / 2) * 3) % 4);
        if (kind == 1 || ((x / 4 + y / 3) % 10) == 0)
            m = -1;
        const uint16_t n = kind == 2 ? uint16_t(0) : counts[next() % 4];
        in.materials[p] = m;
        in.map[p] = n;
        float nx = unit() - 0.5f, ny = unit() - 0.5f, nz = 0.25f + unit();
        if (next() % 8 == 0)
            nz = -nz; /* a normal that faces away from its neighbours' */
        const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
        for (int c = 0; c < 3; c++) {
            const float f = n == 0 ? 0.0f : (next() % 16 == 0 ? 0.0f : unit() * 4.0f);
            in.frame[3 * p + c] = f;
            /* a second moment around the mean's square, sometimes below it (the estimate's max(., 0) clamps that) */
            in.moments[3 * p + c] = n == 0 ? 0.0f : f * f * (0.75f + unit());
            in.positions[3 * p + c] = m < 0 ? 0.0f : (c == 2 ? -2.0f - unit() : (c == 0 ? float(x) : float(y)) * 0.03125f + unit() * 0.0078125f);
        }
        if (next() % 32 == 0 && p > 0 && m >= 0)
            for (int c = 0; c < 3; c++)
                in.positions[3 * p + c] = in.positions[3 * (p - 1) + c]; /* two taps at one point: dd == 0 */
        in.normals[3 * p] = m < 0 ? 0.0f : nx / len;
        in.normals[3 * p + 1] = m < 0 ? 0.0f : ny / len;
        in.normals[3 * p + 2] = m < 0 ? 0.0f : nz / len;
    }
    return in;
}

int main(int argc, char** argv)
{
    static const uint32_t sizes[5][2] = { { 1, 1 }, { 1, 7 }, { 5, 3 }, { 33, 9 }, { 130, 70 } };
    static const char* kinds[3] = { "mixed", "sky", "unsampled" };
    const wptdn::Params params = { 1.0f, 0.1f * 0.1f, 7u };
    unsigned long long failures = 0;
    bool first = true;
    printf("{\n");
    for (int kind = 0; kind < 3; kind++)
        for (const auto& size : sizes) {
            const uint32_t width = size[0], height = size[1];
            const size_t pixels = size_t(width) * height;
            const Inputs in = make(width, height, kind);
            const std::string name = std::string(kinds[kind]) + "_" + std::to_string(width) + "x" + std::to_string(height);
            if (argc > 1) {
                FILE* f = fopen((std::string(argv[1]) + "/" + name + ".bin").c_str(), "wb");
                if (!f) {
                    fprintf(stderr, "cannot write into %s\n", argv[1]);
                    return 2;
                }
                fwrite(in.frame.data(), 4, pixels * 3, f);
                fwrite(in.moments.data(), 4, pixels * 3, f);
                fwrite(in.positions.data(), 4, pixels * 3, f);
                fwrite(in.normals.data(), 4, pixels * 3, f);
                fwrite(in.materials.data(), 4, pixels, f);
                fwrite(in.map.data(), 2, pixels, f);
                fclose(f);
            }
            for (uint32_t iterations = 0; iterations <= wptdn::ITERATIONS_MAX; iterations++) {
                std::vector<wptdn::Rec> scratch(pixels * 4);
                std::vector<float> out(pixels * 3, -1.0f), variance(pixels, -1.0f);
                wptdn::denoiseHost(in.frame.data(), in.moments.data(), in.map.data(), in.positions.data(), in.normals.data(),
                        in.materials.data(), width, height, params, iterations, scratch.data(), out.data(), variance.data());
                /* the same without the variance plane */
                std::vector<float> alone(pixels * 3, -1.0f);
                wptdn::denoiseHost(in.frame.data(), in.moments.data(), in.map.data(), in.positions.data(), in.normals.data(),
                        in.materials.data(), width, height, params, iterations, scratch.data(), alone.data(), nullptr);
                bool good = memcmp(out.data(), alone.data(), pixels * 12) == 0;
                for (size_t k = 0; k < pixels * 3; k++)
                    good = good && std::isfinite(out[k]);
                for (size_t k = 0; k < pixels; k++)
                    good = good && std::isfinite(variance[k]) && variance[k] >= 0.0f;
                if (iterations == 0)
                    good = good && memcmp(out.data(), in.frame.data(), pixels * 12) == 0;
                if (!good && failures++ < 5)
                    fprintf(stderr, "BROKEN: %s with %u iterations\n", name.c_str(), iterations);
                printf("%s  \"%s_i%u\": [\"%016llx\", \"%016llx\"]", first ? "" : ",\n", name.c_str(), iterations,
                        (unsigned long long)digest(out.data(), pixels * 3), (unsigned long long)digest(variance.data(), pixels));
                first = false;
            }
        }
    printf("\n}\n");
    if (failures)
        fprintf(stderr, "%llu failures\n", failures);
    return failures == 0 ? 0 : 1;
}
