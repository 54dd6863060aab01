/*
 * denoise_demodulated_check.cpp -- the demodulated form of wurblpt_amd/csrc/wpt_denoise.h on its own: compiled outside the
 * library, without a header of HIP, with -fsanitize=address,undefined, and run as a program
 * (tests/test_denoise_demodulated_host.py).  Every buffer has exactly the size the interface promises to stay within, so a read
 * or write past it stops the program.
 *   frames (width x height) 1x1, 1x7, 5x3, 33x9, 130x70, each with 0, 1, 3 and 8 iterations and in the three kinds of
 *   tests/denoise_check.cpp ("mixed", "sky", "unsampled"); the albedo's channels are 0, below the floor, the floor itself or
 *   anything up to 1, a tenth of the pixels emit, some of them more than the frame holds (u < 0)
 * Checked here: every output is finite, no variance is negative, the variance plane changes nothing, zero iterations give
 * (frame - emission) / d * d + emission.
 * usage: denoise_demodulated_check [DIRECTORY]
 * Prints one JSON object: "<kind>_<width>x<height>_i<iterations>" -> [digest of the frame, digest of the variance plane], the
 * digest of tests/denoise_check.cpp; the library's host entry must reproduce them.  With a DIRECTORY, the inputs of every frame
 * are left there as <kind>_<width>x<height>.bin: frame, moments, positions, normals, albedo, emission (3 floats per pixel each),
 * materials (int32), sample-count map (uint16).
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_denoise.h"

static uint64_t state = 0x2545f4914f6cdd1dull;
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
    std::vector<float> frame, moments, positions, normals, albedo, emission;
    std::vector<int32_t> materials;
    std::vector<uint16_t> map;
};

/* kind 0: mixed, 1: sky, 2: unsampled */
static Inputs make(uint32_t width, uint32_t height, int kind, float albedoFloor)
{
    const size_t pixels = size_t(width) * height;
    Inputs in;
    for (std::vector<float>* a : { &in.frame, &in.moments, &in.positions, &in.normals, &in.albedo, &in.emission })
        a->resize(pixels * 3);
    in.materials.resize(pixels);
    in.map.resize(pixels);
    static const uint16_t counts[4] = { 0, 1, 2, 5 };
    for (size_t p = 0; p < pixels; p++) {
        const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
        int32_t m = int32_t(((x / 3) * 7 + (y / 2) * 3) % 4);
        if (kind == 1 || ((x / 4 + y / 3) % 10) == 0)
            m = -1;
        const uint16_t n = kind == 2 ? uint16_t(0) : counts[next() % 4];
        in.materials[p] = m;
        in.map[p] = n;
        float nx = unit() - 0.5f, ny = unit() - 0.5f, nz = 0.25f + unit();
        if (next() % 8 == 0)
            nz = -nz;
        const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
        const bool emits = next() % 10 == 0;
        for (int c = 0; c < 3; c++) {
            const float f = n == 0 ? 0.0f : (next() % 16 == 0 ? 0.0f : unit() * 4.0f);
            in.frame[3 * p + c] = f;
            in.moments[3 * p + c] = n == 0 ? 0.0f : f * f * (0.75f + unit());
            in.positions[3 * p + c] = m < 0 ? 0.0f : (c == 2 ? -2.0f - unit() : (c == 0 ? float(x) : float(y)) * 0.03125f + unit() * 0.0078125f);
            const uint32_t pick = next() % 8;
            in.albedo[3 * p + c] = m < 0 ? 0.0f : (pick == 0 ? 0.0f : (pick == 1 ? albedoFloor * 0.5f : (pick == 2 ? albedoFloor : unit())));
            /* an emitter's own light: usually part of the frame's value, sometimes more than all of it */
            in.emission[3 * p + c] = emits ? (next() % 4 == 0 ? f + unit() : f * unit()) : 0.0f;
        }
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
    static const uint32_t iterationCounts[4] = { 0, 1, 3, 8 };
    const wptdn::Params params = { 1.0f, 0.1f * 0.1f, 7u };
    const float albedoFloor = wptdn::k_albedoFloorDefault;
    unsigned long long failures = 0;
    bool first = true;
    printf("{\n");
    for (int kind = 0; kind < 3; kind++)
        for (const auto& size : sizes) {
            const uint32_t width = size[0], height = size[1];
            const size_t pixels = size_t(width) * height;
            const Inputs in = make(width, height, kind, albedoFloor);
            const std::string name = std::string(kinds[kind]) + "_" + std::to_string(width) + "x" + std::to_string(height);
            if (argc > 1) {
                FILE* f = fopen((std::string(argv[1]) + "/" + name + ".bin").c_str(), "wb");
                if (!f) {
                    fprintf(stderr, "cannot write into %s\n", argv[1]);
                    return 2;
                }
                for (const std::vector<float>* a : { &in.frame, &in.moments, &in.positions, &in.normals, &in.albedo, &in.emission })
                    fwrite(a->data(), 4, pixels * 3, f);
                fwrite(in.materials.data(), 4, pixels, f);
                fwrite(in.map.data(), 2, pixels, f);
                fclose(f);
            }
            for (const uint32_t iterations : iterationCounts) {
                std::vector<wptdn::Rec> scratch(pixels * 4);
                std::vector<float> out(pixels * 3, -1.0f), variance(pixels, -1.0f);
                wptdn::denoiseDemodulatedHost(in.frame.data(), in.moments.data(), in.map.data(), in.positions.data(), in.normals.data(),
                        in.materials.data(), in.albedo.data(), in.emission.data(), width, height, params, iterations, albedoFloor,
                        scratch.data(), out.data(), variance.data());
                /* the same without the variance plane */
                std::vector<float> alone(pixels * 3, -1.0f);
                wptdn::denoiseDemodulatedHost(in.frame.data(), in.moments.data(), in.map.data(), in.positions.data(), in.normals.data(),
                        in.materials.data(), in.albedo.data(), in.emission.data(), width, height, params, iterations, albedoFloor,
                        scratch.data(), alone.data(), nullptr);
                bool good = memcmp(out.data(), alone.data(), pixels * 12) == 0;
                for (size_t k = 0; k < pixels * 3; k++)
                    good = good && std::isfinite(out[k]);
                for (size_t k = 0; k < pixels; k++)
                    good = good && std::isfinite(variance[k]) && variance[k] >= 0.0f;
                if (iterations == 0)
                    for (size_t k = 0; k < pixels * 3; k++) {
                        const float d = in.albedo[k] >= albedoFloor ? in.albedo[k] : 1.0f;
                        const float u = (in.frame[k] - in.emission[k]) / d;
                        const float back = u * d + in.emission[k];
                        good = good && memcmp(&back, &out[k], 4) == 0;
                    }
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
