/*
 * image_ops_check.cpp -- wpt_image_ops.h on its own: no library, no header of HIP, every buffer exactly as large as the interface
 * promises, so that the address and undefined-behaviour sanitizers see every access (tests/test_image_ops_host.py builds this
 * with -fsanitize=address,undefined and runs it as a program).
 *   random sizes from 1 x 1 up, 1 to 4 components: resample to another random size; warp both ways through no lens and the three
 *   models, through a lens that throws coordinates far outside the image (finite: they wrap) and through one whose coordinates
 *   overflow (not finite: the pixel must be zeros); distance to coordinates likewise; direct samples at huge, infinite and NaN
 *   coordinates;
 *   despeckle at three factors on the same sizes and on the degenerate shapes 1 x 1, 1 x N, N x 1, 2 x 2.
 * usage: image_ops_check DIRECTORY.  Leaves each input in DIRECTORY (image_K.bin, rgb_K.bin) and prints one JSON object: the
 * images' sizes and the digests of all outputs (tests/golden/image_ops_digests.json); the test runs the library's host entries on
 * the inputs left and expects the same digests.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_image_ops.h"

static void require(bool ok, const char* what)
{
    if (!ok) {
        fprintf(stderr, "image_ops_check: %s\n", what);
        exit(1);
    }
}

static uint32_t step(uint32_t& state)
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

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

static std::string g_digests;

static void report(const std::string& name, const float* values, size_t count)
{
    char line[160];
    snprintf(line, sizeof(line), "%s\"%s\": \"%016llx\"", g_digests.empty() ? "" : ", ", name.c_str(), digest(values, count));
    g_digests += line;
}

static void leave(const std::string& path, const float* values, size_t count)
{
    FILE* f = fopen(path.c_str(), "wb");
    require(f != nullptr && fwrite(values, sizeof(float), count, f) == count, "cannot write an input");
    fclose(f);
}

/* the lens part of a camera record from a frustum and coefficients (optics.hpp:86-99, 170-173), as host.lens_camera makes it */
static wptlens::Coeffs lens(uint32_t type, float k1, float k2, float k3, float p1, float p2)
{
    const float l = -0.625f, r = 0.75f, b = -0.1875f, t = 0.15625f;
    wptlens::Coeffs c = {};
    c.type = type;
    c.cx = l / (l - r);
    c.cy = b / (b - t);
    c.fx = 1.0f / (r - l);
    c.fy = 1.0f / (t - b);
    c.ifx = r - l;
    c.ify = t - b;
    c.k1 = k1; c.k2 = k2; c.k3 = k3; c.p1 = p1; c.p2 = p2;
    if (type == WPT_DISTORTION_RADIAL_ONLY) {
        c.b1 = -k1;
        c.b2 = 3.0f * k1 * k1 - k2;
        c.b3 = -12.0f * k1 * k1 * k1 + 8.0f * k1 * k2 - k3;
        c.b4 = 55.0f * k1 * k1 * k1 * k1 - 55.0f * k1 * k1 * k2 + 5.0f * k2 * k2 + 10.0f * k1 * k3;
    }
    return c;
}

int main(int argc, char* argv[])
{
    require(argc == 2, "usage: image_ops_check DIRECTORY");
    const std::string dir = argv[1];
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct NamedLens { const char* name; wptlens::Coeffs c; };
    const NamedLens lenses[6] = {
        { "none", lens(WPT_DISTORTION_NONE, 0, 0, 0, 0, 0) },
        { "radial_and_planar", lens(WPT_DISTORTION_RADIAL_AND_PLANAR, 0.5f, 0.125f, 0.0f, 0.03125f, -0.015625f) },
        { "radial_only", lens(WPT_DISTORTION_RADIAL_ONLY, 0.375f, 0.0625f, 0.015625f, 0.0f, 0.0f) },
        { "opencv", lens(WPT_DISTORTION_OPENCV, 0.25f, 0.0625f, 0.0078125f, 0.015625f, -0.0078125f) },
        { "far", lens(WPT_DISTORTION_OPENCV, 3.0e6f, 0.0f, 0.0f, 2.0e5f, -1.0e5f) },     /* finite, millions of images away */
        { "overflow", lens(WPT_DISTORTION_OPENCV, 3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f) }, /* infinities and NaN */
    };
    std::string sizes;
    size_t overflowed = 0; /* pixels whose coordinates were not finite */
    uint32_t state = 20240611u;
    const uint32_t fixed[4][2] = { { 1, 1 }, { 1, 9 }, { 11, 1 }, { 2, 2 } };
    for (uint32_t i = 0; i < 10; i++) {
        const uint32_t w = i < 4 ? fixed[i][0] : 1 + step(state) % 40, h = i < 4 ? fixed[i][1] : 1 + step(state) % 24;
        const uint32_t comps = 1 + i % 4;
        const uint32_t w2 = 1 + step(state) % 40, h2 = 1 + step(state) % 24;
        const std::string tag = std::to_string(i);
        char entry[128];
        snprintf(entry, sizeof(entry), "%s[%u, %u, %u, %u, %u]", sizes.empty() ? "" : ", ", w, h, comps, w2, h2);
        sizes += entry;

        /* exact-size buffers on the heap */
        const size_t count = size_t(w) * h * comps;
        std::unique_ptr<float[]> in(new float[count]);
        for (size_t k = 0; k < count; k++)
            in[k] = float(step(state) % 2048u) / 256.0f - 2.0f;
        leave(dir + "/image_" + tag + ".bin", in.get(), count);
        const wptio::Image img = { in.get(), w, h, comps };

        {
            std::unique_ptr<float[]> out(new float[size_t(w2) * h2 * comps]);
            wptio::resampleHost(img, w2, h2, out.get());
            report("resample_" + tag, out.get(), size_t(w2) * h2 * comps);
        }
        for (const NamedLens& l : lenses)
            for (int forward = 0; forward < 2; forward++) {
                std::unique_ptr<float[]> out(new float[count]);
                wptio::warpHost(img, l.c, forward != 0, out.get());
                report(std::string("warp_") + l.name + (forward ? "_forward_" : "_back_") + tag, out.get(), count);
                /* where the coordinates are not finite the pixel is zeros, elsewhere a mix of the image's values */
                size_t zeros = 0;
                for (uint32_t y = 0; y < h; y++)
                    for (uint32_t x = 0; x < w; x++) {
                        float p = (float(x) + 0.5f) * (1.0f / float(w)), q = (float(y) + 0.5f) * (1.0f / float(h));
                        if (forward) {
                            const wptlens::Point r = wptlens::undistortCall(l.c, p, q, w, h);
                            p = r.p;
                            q = r.q;
                        } else {
                            wptlens::distort(l.c, p, q);
                        }
                        const float* px = out.get() + (size_t(y) * w + x) * comps;
                        if (!(std::isfinite(p) && std::isfinite(q))) {
                            zeros++;
                            for (uint32_t c = 0; c < comps; c++)
                                require(px[c] == 0.0f && !std::signbit(px[c]), "a pixel with a coordinate that is not finite is +0");
                        }
                        for (uint32_t c = 0; c < comps; c++)
                            require(px[c] >= -2.0f && px[c] <= 6.0f, "a warped value lies between the image's values");
                    }
                if (std::string(l.name) == "overflow")
                    overflowed += zeros;
                else
                    require(zeros == 0, "the other lenses' coordinates are finite");
            }
        for (int k = 0; k < 6; k += 1 + (k == 0 ? 2 : 0)) /* none, opencv, far, overflow */
            for (int pmd = 0; pmd < 2; pmd++) {
                std::unique_ptr<float[]> out(new float[size_t(w) * h * 3]);
                wptio::coordsHost(img, lenses[k].c, pmd != 0, out.get());
                report(std::string("coords_") + lenses[k].name + (pmd ? "_pmd_" : "_") + tag, out.get(), size_t(w) * h * 3);
            }
        {
            /* single samples at coordinates no lens of the cases reaches */
            const float at[8] = { 1.0e30f, -1.0e30f, 3.4e38f, -0.0f, 1.0f, -1.0e-30f, inf, nan };
            std::unique_ptr<float[]> out(new float[size_t(8) * 8 * comps]);
            for (int a = 0; a < 8; a++)
                for (int b = 0; b < 8; b++) {
                    float* px = out.get() + (size_t(a) * 8 + b) * comps;
                    wptio::sampleOrZero(img, at[a], at[b], px, comps);
                    if (a >= 6 || b >= 6)
                        for (uint32_t c = 0; c < comps; c++)
                            require(px[c] == 0.0f, "a sample at a coordinate that is not finite is 0");
                }
            report("samples_" + tag, out.get(), size_t(8) * 8 * comps);
        }
        {
            /* despeckle: the same size as RGB, quiet values with loud ones strewn in */
            std::unique_ptr<float[]> rgb(new float[size_t(w) * h * 3]);
            for (size_t k = 0; k < size_t(w) * h * 3; k++)
                rgb[k] = float(step(state) % 256u) / 256.0f;
            for (size_t p = 0; p < size_t(w) * h; p++)
                if (step(state) % 16u == 0)
                    for (int c = 0; c < 3; c++)
                        rgb[3 * p + c] = 8.0f + float(step(state) % 64u);
            leave(dir + "/rgb_" + tag + ".bin", rgb.get(), size_t(w) * h * 3);
            const float factors[3] = { 1.0f, 1.25f, 4.0f };
            for (int f = 0; f < 3; f++) {
                std::unique_ptr<float[]> out(new float[size_t(w) * h * 3]);
                wptio::despeckleHost(rgb.get(), w, h, factors[f], out.get());
                report("despeckle_f" + std::to_string(f) + "_" + tag, out.get(), size_t(w) * h * 3);
            }
        }
    }
    require(overflowed > 0, "the overflowing lens has coordinates that are not finite");
    printf("{\"sizes\": [%s], \"digests\": {%s}}\n", sizes.c_str(), g_digests.c_str());
    return 0;
}
