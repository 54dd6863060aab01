/*
 * light_mixer.cpp -- relighting after the render: a room with three lamps is rendered ONCE into a SensorRGBLightGroups, which
 * collects, next to the frame, the frame that each lamp alone would give.  mixLightGroups() then weights the lamps' frames into
 * new pictures -- a lamp switched off, dimmed or given another colour -- without tracing another path.  Nothing that steers a
 * path reads an emitted radiance, so each group's frame is exactly (bit for bit) the render of the room in which only that
 * lamp emits; with "check" as the last argument the program renders those rooms as well and counts the bits that differ.
 *
 * Writes <outdir>/frame.pfm, <outdir>/group_N.pfm and <outdir>/mix_{evening,swapped,dimmed}.pfm (linear RGB, rows bottom-up).
 * Build:  g++ -std=c++20 -fopenmp -I include examples/light_mixer.cpp -L wurblpt_amd/lib -lwurblpt_hip -o light_mixer
 * Usage:  light_mixer [width height samplesSqrt outdir [check]]
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <wurblpt/wurblpt.hpp>

using namespace WurblPT;

struct Lamps {
    const Material* warm;
    const Material* cool;
    const Material* spot; /* two-sided: the spot light in front, a black back */
};

/* the room; only == -1: every lamp emits, otherwise lamp `only` alone (the others' emission is 0: the muted twin) */
static Lamps buildRoom(Scene& scene, int only)
{
    const vec3 xAxis(1.0f, 0.0f, 0.0f), yAxis(0.0f, 1.0f, 0.0f);
    auto emits = [only](int lamp, const vec3& e) { return only < 0 || only == lamp ? e : vec3(0.0f); };
    Material* white = scene.take(new MaterialLambertian(vec3(0.73f, 0.72f, 0.69f)));
    Material* red = scene.take(new MaterialLambertian(vec3(0.6f, 0.1f, 0.08f)));
    Material* blue = scene.take(new MaterialLambertian(vec3(0.12f, 0.2f, 0.55f)));
    Material* metal = scene.take(new MaterialGGX(vec3(0.95f, 0.85f, 0.6f), vec2(0.12f)));
    Material* glass = scene.take(new MaterialGlass(vec3(0.15f), 1.5f));
    auto wall = [&](Material* m, const vec3& where, float degrees, const vec3& axis) {
        scene.take(new MeshInstance(scene.take(generateQuad(Transformation(where, toQuat(radians(degrees), axis), vec3(1.0f)))), m));
    };
    wall(white, vec3(0.0f, 0.0f, 0.0f), -90.0f, xAxis);
    wall(white, vec3(0.0f, 2.0f, 0.0f), +90.0f, xAxis);
    wall(white, vec3(0.0f, 1.0f, -1.0f), 0.0f, yAxis);
    wall(red, vec3(-1.0f, 1.0f, 0.0f), +90.0f, yAxis);
    wall(blue, vec3(+1.0f, 1.0f, 0.0f), -90.0f, yAxis);
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(-0.4f, 0.35f, -0.3f), toQuat(radians(20.0f), yAxis), vec3(0.3f, 0.35f, 0.3f)))), metal));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(0.45f, 0.3f, 0.25f), toQuat(radians(-15.0f), yAxis), vec3(0.28f, 0.3f, 0.28f)))), glass));
    Lamps lamps;
    const quat down = toQuat(radians(90.0f), xAxis);
    lamps.warm = scene.take(new LightDiffuse(emits(0, vec3(9.0f, 6.0f, 3.0f))));
    lamps.cool = scene.take(new LightDiffuse(emits(1, vec3(2.5f, 4.0f, 8.0f))));
    lamps.spot = scene.take(new MaterialTwoSided(scene.take(new LightSpot(radians(50.0f), emits(2, vec3(6.0f, 6.0f, 4.5f)))),
                scene.take(new MaterialLambertian(vec3(0.0f)))));
    scene.take(new MeshInstance(scene.take(generateQuad(Transformation(vec3(-0.5f, 1.98f, -0.1f), down, vec3(0.22f)))), lamps.warm), HotSpot);
    scene.take(new MeshInstance(scene.take(generateQuad(Transformation(vec3(+0.5f, 1.98f, 0.2f), down, vec3(0.25f, 0.18f, 1.0f)))), lamps.cool), HotSpot);
    scene.take(new MeshInstance(scene.take(generateQuad(Transformation(vec3(0.0f, 1.5f, -0.98f), quat::null(), vec3(0.2f)))), lamps.spot), HotSpot);
    scene.updateBVH();
    return lamps;
}

static bool writePfm(const std::string& name, const Array<float>& a)
{
    FILE* f = fopen(name.c_str(), "wb");
    if (!f)
        return false;
    fprintf(f, "PF\n%zu %zu\n-1.0\n", a.dimension(0), a.dimension(1)); /* PFM stores rows bottom-up, like the sensor */
    const size_t n = a.dimension(0) * a.dimension(1) * 3;
    const bool ok = fwrite(a.data(), sizeof(float), n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 512;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 384;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 8;
    const std::string outdir = argc > 4 ? argv[4] : ".";
    const bool check = argc > 5 && strcmp(argv[5], "check") == 0;

    Scene scene;
    const Lamps lamps = buildRoom(scene, -1);
    SensorRGBLightGroups sensor(width, height, 3);
    sensor.assign(lamps.warm, 0);
    sensor.assign(lamps.cool, 1);
    sensor.assign(lamps.spot, 2); /* both sides of the two-sided lamp */
    Optics optics(Projection(radians(45.0f), sensor.aspectRatio()), LensDistortion(), LensDepthOfField(0.0f, 1.0f));
    Camera camera(optics, Transformation::fromLookAt(vec3(0.0f, 1.0f, 3.6f), vec3(0.0f, 0.9f, 0.0f), vec3(0.0f, 1.0f, 0.0f)));
    mcpt(sensor, camera, scene, samplesSqrt);

    bool ok = writePfm(outdir + "/frame.pfm", sensor.result());
    for (unsigned int g = 0; g < sensor.groupCount(); g++)
        ok = writePfm(outdir + "/group_" + std::to_string(g) + ".pfm", sensor.group(g)) && ok;
    /* the evening: the warm lamp alone and the spot at a third; the ceiling lamps' colours swapped; everything at a quarter */
    ok = writePfm(outdir + "/mix_evening.pfm", mixLightGroups(sensor, { 1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.33f, 0.33f, 0.33f })) && ok;
    ok = writePfm(outdir + "/mix_swapped.pfm", mixLightGroups(sensor, { 0.28f, 0.67f, 2.7f, 3.6f, 1.5f, 0.375f, 1.0f, 1.0f, 1.0f })) && ok;
    ok = writePfm(outdir + "/mix_dimmed.pfm", mixLightGroups(sensor, { 0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f })) && ok;
    if (!ok) {
        fprintf(stderr, "light_mixer: cannot write to %s\n", outdir.c_str());
        return 1;
    }
    printf("rendered %ux%u with %u spp into the frame and %u light groups on kernel %s\n", width, height, samplesSqrt * samplesSqrt,
            sensor.groupCount(), sensor.group(0).globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    if (check) {
        /* each group's frame against the plain render of the room in which only that lamp emits */
        size_t differing = 0;
        for (int g = 0; g < 3; g++) {
            Scene twin;
            buildRoom(twin, g);
            SensorRGB plain(width, height);
            mcpt(plain, camera, twin, samplesSqrt);
            const size_t n = size_t(width) * height * 3;
            const float* a = static_cast<const float*>(sensor.group(g).data());
            const float* b = static_cast<const float*>(plain.result().data());
            for (size_t i = 0; i < n; i++) {
                uint32_t x, y;
                memcpy(&x, a + i, sizeof(x));
                memcpy(&y, b + i, sizeof(y));
                differing += __builtin_popcount(x ^ y);
            }
        }
        printf("groups against the renders of their muted twins: %zu differing bits\n", differing);
        return differing == 0 ? 0 : 2;
    }
    return 0;
}
