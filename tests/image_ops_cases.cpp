/*
 * image_ops_cases.cpp -- the cases of the image operations (scale, applyLensDistortion, despeckle, cameraSpaceDistanceToCoords,
 * cameraSpaceToPMDSpace), written with the public spellings that marlam/wurblpt and include/ share, so that ONE source runs
 * against both:
 *   against the reference's libwurblpt and the container stand-in of oracle/tgd_standin (oracle/Makefile's flags for ref_frames,
 *   plus -DIMAGE_OPS_CASES_CHECK_COORDINATES) it wrote tests/golden/image_ops/;
 *   against include/ (tests/test_image_ops_host.py) it must write the same two files byte for byte: the drop-in at source level and
 *   bit parity in one go.
 * usage: image_ops_cases DIRECTORY  -> DIRECTORY/index.json and DIRECTORY/data.bin (raw floats; the index gives offsets in floats).
 * Inputs come from seeded integer arithmetic (small dyadic numbers, exact in float).  Floats in the index are their bit patterns.
 *
 * IMAGE_OPS_CASES_CHECK_COORDINATES uses LensDistortion::getHelper / distort / undistort, which only the reference has, to assert
 * that every sampling coordinate of the warp cases is finite and that some leave [0, 1) and wrap.
 */
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <tgd/array.hpp>

#include "wurblpt.hpp"

using namespace WurblPT;

static std::vector<float> g_data;
static std::string g_index;

static void require(bool ok, const char* what)
{
    if (!ok) {
        fprintf(stderr, "image_ops_cases: %s\n", what);
        exit(1);
    }
}

static uint32_t bits(float v)
{
    uint32_t w;
    memcpy(&w, &v, 4);
    return w;
}

static uint32_t step(uint32_t& state)
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

/* values k / 256 in [0, 4) */
static TGD::Array<float> image(size_t width, size_t height, size_t comps, uint32_t seed)
{
    TGD::Array<float> a({ width, height }, comps);
    uint32_t state = seed * 2654435761u + 12345u;
    for (size_t e = 0; e < a.elementCount(); e++)
        for (size_t c = 0; c < comps; c++)
            a[e][c] = float(step(state) % 1024u) / 256.0f;
    return a;
}

static size_t put(const TGD::Array<float>& a)
{
    const size_t at = g_data.size();
    const float* p = static_cast<const float*>(a.data());
    g_data.insert(g_data.end(), p, p + a.elementCount() * a.componentCount());
    return at;
}

struct Lens {
    const char* name;
    int model; /* 0 none, 1 RadialAndPlanar, 2 RadialOnly, 3 OpenCV */
    float k1, k2, k3, p1, p2;
    LensDistortion make() const
    {
        return model == 1 ? LensDistortion(k1, k2, p1, p2) : model == 2 ? LensDistortion(k1, k2, k3)
            : model == 3 ? LensDistortion(k1, k2, k3, p1, p2) : LensDistortion();
    }
};

/* an asymmetric frustum: the principal point is not the image's centre */
static const float k_frustum[4] = { -0.625f, 0.75f, -0.1875f, 0.15625f };

static void entry(const std::string& name, const char* op, const TGD::Array<float>& in, size_t inAt, const TGD::Array<float>& out,
        const Lens* lens, int forward, int pmd, float minFactor)
{
    char line[1024];
    snprintf(line, sizeof(line),
            "%s  {\"name\": \"%s\", \"op\": \"%s\", \"w\": %zu, \"h\": %zu, \"c\": %zu, \"in\": %zu, \"out_w\": %zu, \"out_h\": %zu, \"out_c\": %zu, "
            "\"out\": %zu, \"forward\": %d, \"pmd\": %d, \"min_factor\": %u, \"model\": %d, \"frustum\": [%u, %u, %u, %u], "
            "\"k\": [%u, %u, %u, %u, %u]}",
            g_index.empty() ? "" : ",\n", name.c_str(), op, in.dimension(0), in.dimension(1), in.componentCount(), inAt, out.dimension(0),
            out.dimension(1), out.componentCount(), put(out), forward, pmd, bits(minFactor), lens ? lens->model : 0, bits(k_frustum[0]),
            bits(k_frustum[1]), bits(k_frustum[2]), bits(k_frustum[3]), bits(lens ? lens->k1 : 0.0f), bits(lens ? lens->k2 : 0.0f),
            bits(lens ? lens->k3 : 0.0f), bits(lens ? lens->p1 : 0.0f), bits(lens ? lens->p2 : 0.0f));
    g_index += line;
}

static bool sameBits(const float* a, const float* b, size_t n)
{
    return memcmp(a, b, n * sizeof(float)) == 0;
}

/* a 3 x 3 frame whose centre is a speckle and whose sorted slots 4 and 5 hold `first` and `second` at row-major places 2 and 6 */
static TGD::Array<float> tieFrame(const float* first, const float* second)
{
    TGD::Array<float> a({ size_t(3), size_t(3) }, 3);
    const float grey[9] = { 0.125f, 0.25f, 0.0f, 0.375f, 16.0f, 2.0f, 0.0f, 0.4375f, 3.0f };
    for (size_t e = 0; e < 9; e++)
        for (size_t c = 0; c < 3; c++)
            a[e][c] = e == 2 ? first[c] : e == 6 ? second[c] : grey[e];
    return a;
}

int main(int argc, char* argv[])
{
    require(argc == 2, "usage: image_ops_cases DIRECTORY");
    const Projection projection(k_frustum[0], k_frustum[1], k_frustum[2], k_frustum[3]);

    /* resample: 7 x 5 to wider and flatter, to itself, to one pixel, to narrower and taller; one pixel to 4 x 4 */
    const size_t targets[4][2] = { { 11, 3 }, { 7, 5 }, { 1, 1 }, { 3, 13 } };
    for (size_t comps = 1; comps <= 4; comps++) {
        const TGD::Array<float> in = image(7, 5, comps, 10 + uint32_t(comps));
        const size_t inAt = put(in);
        for (const auto& t : targets)
            entry("resample_c" + std::to_string(comps) + "_" + std::to_string(t[0]) + "x" + std::to_string(t[1]), "resample", in, inAt,
                    scale(in, (unsigned int)t[0], (unsigned int)t[1]), nullptr, 0, 0, 0.0f);
        const TGD::Array<float> one = image(1, 1, comps, 20 + uint32_t(comps));
        entry("resample_c" + std::to_string(comps) + "_1x1_to_4x4", "resample", one, put(one), scale(one, 4, 4), nullptr, 0, 0, 0.0f);
    }

    /* warp, both ways, no lens and the three models: strong enough that corners leave [0, 1) */
    const Lens lenses[4] = {
        { "none", 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f },
        { "radial_and_planar", 1, 0.5f, 0.125f, 0.0f, 0.03125f, -0.015625f },
        { "radial_only", 2, 0.375f, 0.0625f, 0.015625f, 0.0f, 0.0f },
        { "opencv", 3, 0.25f, 0.0625f, 0.0078125f, 0.015625f, -0.0078125f },
    };
    {
        const TGD::Array<float> in = image(33, 9, 3, 30);
        const size_t inAt = put(in);
        const TGD::Array<float> two = image(8, 6, 2, 31);
        const size_t twoAt = put(two);
        for (const Lens& lens : lenses) {
            const LensDistortion distortion = lens.make();
            require(int(distortion.type) == lens.model, "a lens has the model its coefficients ask for");
            size_t outside = 0; /* sampling coordinates outside [0, 1), over both directions */
            for (int forward = 0; forward < 2; forward++) {
#ifdef IMAGE_OPS_CASES_CHECK_COORDINATES
                const LensDistortion::Helper helper = distortion.getHelper(projection, 33, 9);
                for (size_t y = 0; y < 9; y++)
                    for (size_t x = 0; x < 33; x++) {
                        float p = (x + 0.5f) * (1.0f / 33), q = (y + 0.5f) * (1.0f / 9);
                        if (forward)
                            distortion.undistort(p, q, helper);
                        else
                            distortion.distort(p, q, helper);
                        require(std::isfinite(p) && std::isfinite(q), "a sampling coordinate is finite");
                        outside += (p < 0.0f || p >= 1.0f || q < 0.0f || q >= 1.0f) ? 1 : 0;
                    }
#endif
                const std::string name = std::string("warp_") + lens.name + (forward ? "_forward" : "_back");
                entry(name, "warp", in, inAt, forward ? distort(in, distortion, projection) : undistort(in, distortion, projection), &lens,
                        forward, 0, 0.0f);
                entry(name + "_c2", "warp", two, twoAt, applyLensDistortion(two, distortion, projection, forward != 0), &lens, forward, 0, 0.0f);
            }
#ifdef IMAGE_OPS_CASES_CHECK_COORDINATES
            require(lens.model == 0 ? outside == 0 : outside > 0, "some sampling coordinates of a lens leave [0, 1) and wrap");
            fprintf(stderr, "%s: %zu sampling coordinates outside [0, 1)\n", lens.name, outside);
#else
            (void)outside;
#endif
        }
    }

    /* despeckle at three factors */
    {
        std::vector<std::pair<std::string, TGD::Array<float>>> frames;
        frames.push_back({ "1x1", image(1, 1, 3, 40) });
        frames.push_back({ "1x7", image(1, 7, 3, 41) });
        frames.push_back({ "5x3", image(5, 3, 3, 42) });
        TGD::Array<float> constant({ size_t(6), size_t(4) }, 3);
        for (size_t e = 0; e < constant.elementCount(); e++)
            for (size_t c = 0; c < 3; c++)
                constant[e][c] = 0.75f;
        frames.push_back({ "constant", constant });
        /* a quiet 9 x 7 frame (values below 1) with speckles in a corner, on an edge, inside, and two side by side */
        TGD::Array<float> speckled = image(9, 7, 3, 43);
        for (size_t e = 0; e < speckled.elementCount(); e++)
            for (size_t c = 0; c < 3; c++)
                speckled[e][c] *= 0.25f;
        const size_t at[5][2] = { { 0, 0 }, { 4, 6 }, { 3, 3 }, { 6, 2 }, { 7, 2 } };
        for (size_t k = 0; k < 5; k++)
            for (size_t c = 0; c < 3; c++)
                speckled[{ at[k][0], at[k][1] }][c] = 8.0f + float(k) + 0.5f * float(c);
        frames.push_back({ "speckles", speckled });
        /* two colours of one luminance: the blue channel's weight is small enough for its last bits to vanish in the sum */
        const float a[3] = { 0.5f, 0.5f, 0.5f }, b[3] = { 0.5f, 0.5f, 0.5f + 1.0f / 8388608.0f };
        const TGD::Array<float> tie = tieFrame(a, b), tieSwapped = tieFrame(b, a);
        const TGD::Array<float> tieOut = despeckle(tie, 1.25f), tieSwappedOut = despeckle(tieSwapped, 1.25f);
        require(!sameBits(a, b, 3), "the tied pixels differ in colour");
        require(sameBits(tieOut[{ size_t(1), size_t(1) }], a, 3) && sameBits(tieSwappedOut[{ size_t(1), size_t(1) }], b, 3),
                "of two pixels with one luminance astride sorted slot 4 the earlier in row-major order wins: reversing the tie order changes the output");
        frames.push_back({ "tie", tie });
        frames.push_back({ "tie_swapped", tieSwapped });
        const float factors[3] = { 1.0f, 1.25f, 4.0f };
        for (const auto& f : frames) {
            const size_t inAt = put(f.second);
            for (size_t k = 0; k < 3; k++)
                entry("despeckle_" + f.first + "_f" + std::to_string(k), "despeckle", f.second, inAt, despeckle(f.second, factors[k]), nullptr, 0, 0,
                        factors[k]);
        }
        require(!sameBits(static_cast<const float*>(despeckle(speckled, 1.25f).data()), static_cast<const float*>(speckled.data()),
                    speckled.elementCount() * 3), "speckles are removed");
    }

    /* distances to coordinates: with and without a lens, camera space and PMD space, one and three components */
    for (size_t comps = 1; comps <= 3; comps += 2) {
        TGD::Array<float> distances = image(13, 9, comps, 50 + uint32_t(comps));
        for (size_t e = 0; e < distances.elementCount(); e++)
            distances[e][0] += 1.0f;
        const size_t inAt = put(distances);
        for (int l = 0; l < 4; l += 3) {
            const LensDistortion distortion = lenses[l].make();
            const TGD::Array<float> coords = cameraSpaceDistanceToCoords(distances, projection, distortion);
            const std::string name = "coords_c" + std::to_string(comps) + "_" + lenses[l].name;
            entry(name, "coords", distances, inAt, coords, &lenses[l], 0, 0, 0.0f);
            entry(name + "_pmd", "coords", distances, inAt, cameraSpaceToPMDSpace(coords), &lenses[l], 0, 1, 0.0f);
        }
    }

    const std::string dir = argv[1];
    FILE* f = fopen((dir + "/index.json").c_str(), "w");
    require(f != nullptr, "cannot write index.json");
    fprintf(f, "[\n%s\n]\n", g_index.c_str());
    fclose(f);
    f = fopen((dir + "/data.bin").c_str(), "wb");
    require(f != nullptr && fwrite(g_data.data(), sizeof(float), g_data.size(), f) == g_data.size(), "cannot write data.bin");
    fclose(f);
    return 0;
}
