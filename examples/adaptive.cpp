/*
 * adaptive.cpp -- adaptive sampling of a Cornell box with a glass sphere and a GGX box (include/wurblpt/wurblpt.hpp: mcpt() with
 * a sample-count map, samplesSqrtForError).  A pilot render with pilotSqrt^2 samples per pixel and its moment film estimates
 * every pixel's variance; samplesSqrtForError turns that into the sample count each pixel needs for a relative standard error
 * of `relError`; the final render spends exactly those samples.  Each pixel of the final frame is bit for bit the plain render
 * at its own count.  It links libwurblpt_hip.so and nothing else; everything from mcpt() on runs on the GPU.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/adaptive.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o adaptive
 *   ./adaptive [width height pilotSqrt relError maxSqrt outdir]
 *
 * Writes adaptive.png (the final frame, sRGB) and adaptive-map.png (the map: n / maxSqrt taken as a linear grey level and
 * stored sRGB-encoded, as toSRGB stores every image).
 */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <wurblpt/wurblpt.hpp>

using namespace WurblPT;

static void quad(Scene& scene, const Material* m, const vec3& a, const vec3& b, const vec3& c, const vec3& d, const vec3& n,
        HotSpotType hot = ColdSpot)
{
    scene.take(new MeshInstance(scene.take(new Mesh({ a, b, c, d }, { n, n, n, n },
                        { vec2(0.0f, 0.0f), vec2(1.0f, 0.0f), vec2(1.0f, 1.0f), vec2(0.0f, 1.0f) }, { 0, 1, 2, 0, 2, 3 })), m), hot);
}

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 512;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 512;
    const unsigned int pilotSqrt = argc > 3 ? atoi(argv[3]) : 4;
    const double relError = argc > 4 ? atof(argv[4]) : 0.05;
    const unsigned int maxSqrt = argc > 5 ? atoi(argv[5]) : 32;
    const std::string outdir = argc > 6 ? argv[6] : ".";

    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.725f, 0.71f, 0.68f)));
    Material* red = scene.take(new MaterialLambertian(vec3(0.63f, 0.065f, 0.05f)));
    Material* green = scene.take(new MaterialLambertian(vec3(0.14f, 0.45f, 0.091f)));
    Material* light = scene.take(new LightDiffuse(vec3(4.0f)));
    Material* metal = scene.take(new MaterialGGX(vec3(1.0f), vec2(0.04f)));
    Material* glass = scene.take(new MaterialGlass(vec3(0.1f), 1.5f));
    quad(scene, red, vec3(-1, 0, 1), vec3(-1, 0, -1), vec3(-1, 2, -1), vec3(-1, 2, 1), vec3(1, 0, 0));
    quad(scene, green, vec3(1, 0, -1), vec3(1, 0, 1), vec3(1, 2, 1), vec3(1, 2, -1), vec3(-1, 0, 0));
    quad(scene, white, vec3(-1, 0, 1), vec3(1, 0, 1), vec3(1, 0, -1), vec3(-1, 0, -1), vec3(0, 1, 0));
    quad(scene, white, vec3(-1, 2, 1), vec3(-1, 2, -1), vec3(1, 2, -1), vec3(1, 2, 1), vec3(0, -1, 0));
    quad(scene, white, vec3(-1, 0, -1), vec3(1, 0, -1), vec3(1, 2, -1), vec3(-1, 2, -1), vec3(0, 0, 1));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(-0.4f, 0.4f, -0.3f), toQuat(radians(20.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f, 0.4f, 0.3f)))), metal));
    scene.take(new MeshInstance(scene.take(generateSphere(Transformation(vec3(0.45f, 0.3f, 0.3f), quat::null(), vec3(0.3f)))), glass));
    quad(scene, light, vec3(-0.24f, 1.98f, 0.16f), vec3(-0.24f, 1.98f, -0.22f), vec3(0.23f, 1.98f, -0.22f), vec3(0.23f, 1.98f, 0.16f),
            vec3(0, -1, 0), HotSpot);
    scene.updateBVH();
    const Camera camera(Optics(Projection(radians(50.0f), float(width) / height)),
            Transformation::fromLookAt(vec3(0.0f, 1.0f, 3.2f), vec3(0.0f, 1.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f)));

    /* 1. the pilot, with its moment film: every pixel at pilotSqrt^2 samples */
    SensorRGB pilot(width, height);
    Array<float> moments;
    mcpt(pilot, camera, scene, std::vector<uint16_t>(size_t(width) * height, uint16_t(pilotSqrt)), 0.0f, 0.0f, Parameters(), &moments);
    /* 2. the map: the count each pixel needs for relError (values below 0.05 count as 0.05) */
    const std::vector<uint16_t> map = samplesSqrtForError(pilot.result(), moments, pilotSqrt, relError, 1, maxSqrt, 0.05);
    /* 3. the final render with the map (the pilot's samples are not merged: each pixel stays the plain render at its count) */
    SensorRGB sensor(width, height);
    mcpt(sensor, camera, scene, map);

    Array<float> mapImage(width, height, 3);
    for (size_t i = 0; i < map.size(); i++)
        for (int c = 0; c < 3; c++)
            mapImage[i][c] = float(map[i]) / float(maxSqrt);
    const Array<float>& hdr = sensor.result();
    std::string error;
    if (!saveImage(toSRGB(uniformRationalQuantization(hdr, maxLuminance(hdr), 4.0f)), outdir + "/adaptive.png", &error)
            || !saveImage(toSRGB(mapImage), outdir + "/adaptive-map.png", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    printf("rendered %ux%u adaptively: %s samples in all (uniform at %u: %llu) on kernel %s\n", width, height,
            hdr.globalTagList().value("WURBLPT/SAMPLES_TOTAL").c_str(), maxSqrt,
            static_cast<unsigned long long>(maxSqrt) * maxSqrt * width * height, hdr.globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    return 0;
}
