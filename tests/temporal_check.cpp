/*
 * temporal_check.cpp -- wurblpt_amd/csrc/wpt_temporal.h (and wpt_denoise.h under it) on its own: compiled outside the library,
 * without a header of HIP, with -fsanitize=address,undefined, and run as a program (tests/test_temporal_host.py).  Every buffer
 * has exactly the size the interface promises to stay within, so a read or write past it stops the program.
 *   frames (width x height) 1x1, 1x7, 5x3, 33x9, 130x70, each a chain of three frames in five kinds of motion:
 *   "none" (NULL offsets), "zero" (offsets 0), "whole" (every frame's guide is the one before shifted by (3, -2), with offsets that
 *   say so), "fractional" (the offset (0.37, -1.61)) and "random" (per pixel from +-3, one in sixteen NaN, infinite or far outside
 *   the frame).  Several materials, a tenth of the pixels sky, n_p in {0, 1, 2, 5}.
 * Checked here: every word of a history is finite, no variance and no length is negative, no length exceeds the frame count, the
 * length plane is the history's, the previous history is not written, the filter leaves the history alone.
 * usage: temporal_check [DIRECTORY]
 * Prints one JSON object: "<kind>_<width>x<height>" -> [the digests of the three histories (every word, 12 per pixel), then of the
 * frame and of the variance plane that three iterations of the filter make of the last one], a digest being tests/denoise_check.cpp's
 * (tests/golden/temporal_digests.json holds these lines; the library's host entries must reproduce them).  With a DIRECTORY, the
 * inputs of frame k are left there as <kind>_<width>x<height>_f<k>.bin: frame, moments, positions, normals (3 floats per pixel
 * each), materials (int32), pixel offsets (2 floats), camera offsets (3 floats), sample-count map (uint16).
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_temporal.h"
#include "../wurblpt_amd/csrc/wpt_denoise.h"

using wptdn::Rec;

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

struct Guide {
    std::vector<float> positions, normals;
    std::vector<int32_t> materials;
};

struct Frame {
    std::vector<float> frame, moments, pixelOffsets, cameraOffsets;
    std::vector<uint16_t> map;
};

/* materials in patches of a few pixels, a tenth of them sky; each material a plane seen at a slant with a rough surface and
 * normals a few degrees around its own */
static Guide makeGuide(uint32_t width, uint32_t height)
{
    static const float base[4][3] = { { 0.1f, 0.2f, 1.0f }, { 0.6f, 0.0f, 0.8f }, { -0.3f, 0.3f, 0.9f }, { 0.0f, -0.5f, 0.85f } };
    const size_t pixels = size_t(width) * height;
    Guide g;
    g.positions.resize(pixels * 3);
    g.normals.resize(pixels * 3);
    g.materials.resize(pixels);
    for (size_t p = 0; p < pixels; p++) {
        const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
        int32_t m = int32_t(((x / 3) * 7 + (y / 2) * 3) % 4);
        if (((x / 4 + y / 3) % 10) == 0)
            m = -1;
        g.materials[p] = m;
        float n[3];
        for (int c = 0; c < 3; c++)
            n[c] = m < 0 ? 0.0f : base[m][c] + (unit() - 0.5f) * 0.1f;
        const float len = m < 0 ? 1.0f : std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int c = 0; c < 3; c++)
            g.normals[3 * p + c] = n[c] / len;
        g.positions[3 * p] = m < 0 ? 0.0f : float(x) * 0.03125f;
        g.positions[3 * p + 1] = m < 0 ? 0.0f : float(y) * 0.03125f;
        g.positions[3 * p + 2] = m < 0 ? 0.0f : -2.0f - 0.5f * float(m) - 0.01f * float(x) - 0.02f * float(y) + (unit() - 0.5f) * 0.004f;
    }
    return g;
}

/* the guide whose pixel (x, y) shows what g shows at (x + ox, y + oy); its own pixel where that lies outside the frame */
static Guide shiftGuide(const Guide& g, uint32_t width, uint32_t height, int ox, int oy)
{
    Guide s = g;
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const int sx = int(x) + ox, sy = int(y) + oy;
            if (sx < 0 || sy < 0 || sx >= int(width) || sy >= int(height))
                continue;
            const size_t p = size_t(y) * width + x, q = size_t(sy) * width + size_t(sx);
            s.materials[p] = g.materials[q];
            for (int c = 0; c < 3; c++) {
                s.positions[3 * p + c] = g.positions[3 * q + c];
                s.normals[3 * p + c] = g.normals[3 * q + c];
            }
        }
    return s;
}

/* kind 0: none, 1: zero, 2: whole, 3: fractional, 4: random */
static Frame makeFrame(uint32_t width, uint32_t height, int kind)
{
    static const uint16_t counts[4] = { 0, 1, 2, 5 };
    const size_t pixels = size_t(width) * height;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    Frame f;
    f.frame.resize(pixels * 3);
    f.moments.resize(pixels * 3);
    f.pixelOffsets.assign(pixels * 2, 0.0f);
    f.cameraOffsets.assign(pixels * 3, 0.0f);
    f.map.resize(pixels);
    for (size_t p = 0; p < pixels; p++) {
        const uint16_t n = counts[next() % 4];
        f.map[p] = n;
        for (int c = 0; c < 3; c++) {
            const float v = n == 0 ? 0.0f : (next() % 16 == 0 ? 0.0f : unit() * 4.0f);
            f.frame[3 * p + c] = v;
            f.moments[3 * p + c] = n == 0 ? 0.0f : v * v * (0.75f + unit());
        }
        float dx = 0.0f, dy = 0.0f;
        if (kind == 2) {
            dx = 3.0f;
            dy = -2.0f;
        } else if (kind == 3) {
            dx = 0.37f;
            dy = -1.61f;
        } else if (kind == 4) {
            dx = (unit() - 0.5f) * 6.0f;
            dy = (unit() - 0.5f) * 6.0f;
        }
        f.pixelOffsets[2 * p] = dx;
        f.pixelOffsets[2 * p + 1] = dy;
        if (kind >= 3) {
            /* on the guide's slanted planes a point seen (dx, dy) pixels away lay here */
            f.cameraOffsets[3 * p] = dx * 0.03125f;
            f.cameraOffsets[3 * p + 1] = dy * 0.03125f;
            f.cameraOffsets[3 * p + 2] = -0.01f * dx - 0.02f * dy;
        }
        if (kind == 4 && next() % 16 == 0) {
            const uint32_t what = next() % 4;
            f.pixelOffsets[2 * p] = what == 0 ? nan : (what == 1 ? inf : (what == 2 ? dx : 1e6f));
            f.pixelOffsets[2 * p + 1] = what == 0 ? nan : (what == 1 ? dy : (what == 2 ? -inf : -3e5f));
            f.cameraOffsets[3 * p + 2] = what == 3 ? nan : f.cameraOffsets[3 * p + 2]; /* the offsets may be anything */
        }
    }
    return f;
}

int main(int argc, char** argv)
{
    static const uint32_t sizes[5][2] = { { 1, 1 }, { 1, 7 }, { 5, 3 }, { 33, 9 }, { 130, 70 } };
    static const char* kinds[5] = { "none", "zero", "whole", "fractional", "random" };
    const wpttm::Params rule = { 32.0f, 0.9f, 0.02f * 0.02f };
    const wptdn::Params filter = { 1.0f, 0.1f * 0.1f, 7u };
    unsigned long long failures = 0;
    bool first = true;
    printf("{\n");
    for (const auto& size : sizes)
        for (int kind = 0; kind < 5; kind++) {
            const uint32_t width = size[0], height = size[1];
            const size_t pixels = size_t(width) * height;
            const std::string name = std::string(kinds[kind]) + "_" + std::to_string(width) + "x" + std::to_string(height);
            Guide guide = makeGuide(width, height);
            std::vector<Rec> histories[2] = { std::vector<Rec>(pixels * 3), std::vector<Rec>(pixels * 3) };
            unsigned long long digests[5];
            bool good = true;
            for (int k = 0; k < 3; k++) {
                if (kind == 2 && k > 0)
                    guide = shiftGuide(guide, width, height, 3, -2);
                const Frame f = makeFrame(width, height, kind);
                if (argc > 1) {
                    FILE* file = fopen((std::string(argv[1]) + "/" + name + "_f" + std::to_string(k) + ".bin").c_str(), "wb");
                    if (!file) {
                        fprintf(stderr, "cannot write into %s\n", argv[1]);
                        return 2;
                    }
                    fwrite(f.frame.data(), 4, pixels * 3, file);
                    fwrite(f.moments.data(), 4, pixels * 3, file);
                    fwrite(guide.positions.data(), 4, pixels * 3, file);
                    fwrite(guide.normals.data(), 4, pixels * 3, file);
                    fwrite(guide.materials.data(), 4, pixels, file);
                    fwrite(f.pixelOffsets.data(), 4, pixels * 2, file);
                    fwrite(f.cameraOffsets.data(), 4, pixels * 3, file);
                    fwrite(f.map.data(), 2, pixels, file);
                    fclose(file);
                }
                const std::vector<Rec>& prev = histories[(k + 1) & 1];
                std::vector<Rec>& out = histories[k & 1];
                const std::vector<Rec> before = prev;
                std::vector<float> length(pixels, -1.0f);
                wpttm::accumulateHost(f.frame.data(), f.moments.data(), f.map.data(), guide.positions.data(), guide.normals.data(),
                        guide.materials.data(), kind == 0 ? nullptr : f.pixelOffsets.data(), kind == 0 ? nullptr : f.cameraOffsets.data(),
                        k == 0 ? nullptr : prev.data(), width, height, rule, out.data(), length.data());
                /* the same without the length plane */
                std::vector<Rec> alone(pixels * 3);
                wpttm::accumulateHost(f.frame.data(), f.moments.data(), f.map.data(), guide.positions.data(), guide.normals.data(),
                        guide.materials.data(), kind == 0 ? nullptr : f.pixelOffsets.data(), kind == 0 ? nullptr : f.cameraOffsets.data(),
                        k == 0 ? nullptr : prev.data(), width, height, rule, alone.data(), nullptr);
                good = good && memcmp(out.data(), alone.data(), pixels * 48) == 0 && memcmp(before.data(), prev.data(), pixels * 48) == 0;
                for (size_t p = 0; p < pixels; p++) {
                    const Rec &a = out[p], &b = out[pixels + p], &c = out[2 * pixels + p];
                    good = good && std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z) && std::isfinite(b.x) && std::isfinite(b.y)
                        && std::isfinite(b.z) && std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.z);
                    good = good && c.w >= 0.0f && std::isfinite(c.w) && b.w >= 0.0f && b.w <= float(k + 1) && length[p] == b.w;
                }
                digests[k] = digest(&out[0].x, pixels * 12);
            }
            const std::vector<Rec>& last = histories[0];
            const std::vector<Rec> before = last;
            std::vector<Rec> scratch(pixels * 2);
            std::vector<float> frame(pixels * 3, -1.0f), variance(pixels, -1.0f);
            wpttm::denoiseHistoryHost(last.data(), width, height, filter, 3, scratch.data(), frame.data(), variance.data());
            good = good && memcmp(before.data(), last.data(), pixels * 48) == 0;
            /* no iterations need no scratch and return the accumulated frame's own bits */
            std::vector<float> plain(pixels * 3, -1.0f);
            wpttm::denoiseHistoryHost(last.data(), width, height, filter, 0, nullptr, plain.data(), nullptr);
            for (size_t p = 0; p < pixels; p++)
                good = good && memcmp(&plain[3 * p], &last[2 * pixels + p].x, 12) == 0 && std::isfinite(variance[p]) && variance[p] >= 0.0f;
            for (size_t k = 0; k < pixels * 3; k++)
                good = good && std::isfinite(frame[k]);
            digests[3] = digest(frame.data(), pixels * 3);
            digests[4] = digest(variance.data(), pixels);
            if (!good && failures++ < 5)
                fprintf(stderr, "BROKEN: %s\n", name.c_str());
            printf("%s  \"%s\": [\"%016llx\", \"%016llx\", \"%016llx\", \"%016llx\", \"%016llx\"]", first ? "" : ",\n", name.c_str(), digests[0],
                    digests[1], digests[2], digests[3], digests[4]);
            first = false;
        }
    printf("\n}\n");
    if (failures)
        fprintf(stderr, "%llu failures\n", failures);
    return failures == 0 ? 0 : 1;
}
