/*
 * light_in_flight.cpp -- a light-propagation video of the Cornell box in one render: a SensorRGBTransient collects, next to
 * the frame, the light of every optical path length bin [start + k * width, start + (k + 1) * width).  Slice k shows where
 * the light is that has travelled that far from the light source to the camera; played in order, the slices show the light
 * spreading through the box.  The whole video costs one pass over the paths, not one render per slice.
 *
 * The box is the one of the reference's wurblpt-cornellbox application (GGX metal tall box, glass short box).
 * Writes <outdir>/frame.pfm and <outdir>/slice_NNN.pfm (linear RGB, rows bottom-up like the sensor).
 * Build:  g++ -std=c++20 -fopenmp -I include examples/light_in_flight.cpp -L wurblpt_amd/lib -lwurblpt_hip -o light_in_flight
 * Usage:  light_in_flight [width height samplesSqrt slices startPathLen sliceWidth outdir]
 */
#include <cstdio>
#include <cstdlib>
#include <string>

#include <wurblpt/wurblpt.hpp>

using namespace WurblPT;

static void quad(Scene& scene, const Material* m, const float (&p)[4][3], const vec3& n, HotSpotType hot = ColdSpot,
        const vec2 (&tc)[4] = { vec2(0.0f, 0.0f), vec2(1.0f, 0.0f), vec2(1.0f, 1.0f), vec2(0.0f, 1.0f) })
{
    scene.take(new MeshInstance(scene.take(new Mesh({ vec3(p[0][0], p[0][1], p[0][2]), vec3(p[1][0], p[1][1], p[1][2]),
                        vec3(p[2][0], p[2][1], p[2][2]), vec3(p[3][0], p[3][1], p[3][2]) }, { n, n, n, n },
                        { tc[0], tc[1], tc[2], tc[3] }, { 0, 1, 2, 0, 2, 3 })), m), hot);
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
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 512;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 8;
    const unsigned int slices = argc > 4 ? atoi(argv[4]) : 64;
    const float start = argc > 5 ? float(atof(argv[5])) : 2.0f;
    const float sliceWidth = argc > 6 ? float(atof(argv[6])) : 0.125f;
    const std::string outdir = argc > 7 ? argv[7] : ".";

    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.725f, 0.71f, 0.68f)));
    Material* red = scene.take(new MaterialLambertian(vec3(0.63f, 0.065f, 0.05f)));
    Material* green = scene.take(new MaterialLambertian(vec3(0.14f, 0.45f, 0.091f)));
    Material* light = scene.take(new LightDiffuse(vec3(4.0f)));
    Material* metal = scene.take(new MaterialGGX(vec3(1.0f), vec2(0.04f)));
    Material* glass = scene.take(new MaterialGlass(vec3(0.2f), 1.5f));
    { /* left wall: its normals lean a little */
        const float p[4][3] = { { -1.01f, 0.0f, 0.99f }, { -0.99f, 0.0f, -1.04f }, { -1.02f, 1.99f, -1.04f }, { -1.02f, 1.99f, 0.99f } };
        scene.take(new MeshInstance(scene.take(new Mesh({ vec3(p[0][0], p[0][1], p[0][2]), vec3(p[1][0], p[1][1], p[1][2]),
                            vec3(p[2][0], p[2][1], p[2][2]), vec3(p[3][0], p[3][1], p[3][2]) },
                            { vec3(0.9999874f, 0.005025057f, 0.0f), vec3(0.9998379f, 0.01507292f, 0.009850611f),
                              vec3(0.9999874f, 0.005025057f, 0.0f), vec3(0.9999874f, 0.005025057f, 0.0f) },
                            { vec2(0.0f, 0.0f), vec2(1.0f, 0.0f), vec2(1.0f, 1.0f), vec2(0.0f, 1.0f) }, { 0, 1, 2, 0, 2, 3 })), red));
    }
    const float rightWall[4][3] = { { 1.0f, 0.0f, -1.04f }, { 1.0f, 0.0f, 0.99f }, { 1.0f, 1.99f, 0.99f }, { 1.0f, 1.99f, -1.04f } };
    quad(scene, green, rightWall, vec3(-1.0f, 0.0f, 0.0f));
    const float floor[4][3] = { { -1.01f, 0.0f, 0.99f }, { 1.0f, 0.0f, 0.99f }, { 1.0f, 0.0f, -1.04f }, { -0.99f, 0.0f, -1.04f } };
    quad(scene, white, floor, vec3(0.0f, 1.0f, 0.0f));
    const float ceiling[4][3] = { { -1.02f, 1.99f, 0.99f }, { -1.02f, 1.99f, -1.04f }, { 1.0f, 1.99f, -1.04f }, { 1.0f, 1.99f, 0.99f } };
    quad(scene, white, ceiling, vec3(0.0f, -1.0f, 0.0f));
    const float back[4][3] = { { -0.99f, 0.0f, -1.04f }, { 1.0f, 0.0f, -1.04f }, { 1.0f, 1.99f, -1.04f }, { -1.02f, 1.99f, -1.04f } };
    quad(scene, white, back, vec3(0.0f, 0.0f, 1.0f));
    /* short box (glass): left, right, floor, ceiling, back, front */
    const float s0[4][3] = { { -0.05f, 0.0f, 0.57f }, { -0.05f, 0.6f, 0.57f }, { 0.13f, 0.6f, 0.0f }, { 0.13f, 0.0f, 0.0f } };
    quad(scene, glass, s0, vec3(-0.9535826f, 0.0f, -0.3011314f));
    const float s1[4][3] = { { 0.7f, 0.0f, 0.17f }, { 0.7f, 0.6f, 0.17f }, { 0.53f, 0.6f, 0.75f }, { 0.53f, 0.0f, 0.75f } };
    quad(scene, glass, s1, vec3(0.9596285f, 0.0f, 0.2812705f));
    const float s2[4][3] = { { 0.53f, 0.0f, 0.75f }, { 0.7f, 0.0f, 0.17f }, { 0.13f, 0.0f, 0.0f }, { -0.05f, 0.0f, 0.57f } };
    quad(scene, glass, s2, vec3(0.0f, -1.0f, 0.0f));
    const float s3[4][3] = { { 0.53f, 0.6f, 0.75f }, { 0.7f, 0.6f, 0.17f }, { 0.13f, 0.6f, 0.0f }, { -0.05f, 0.6f, 0.57f } };
    quad(scene, glass, s3, vec3(0.0f, 1.0f, 0.0f));
    const float s4[4][3] = { { 0.13f, 0.0f, 0.0f }, { 0.13f, 0.6f, 0.0f }, { 0.7f, 0.6f, 0.17f }, { 0.7f, 0.0f, 0.17f } };
    quad(scene, glass, s4, vec3(0.2858051f, 0.0f, -0.9582878f));
    const float s5[4][3] = { { 0.53f, 0.0f, 0.75f }, { 0.53f, 0.6f, 0.75f }, { -0.05f, 0.6f, 0.57f }, { -0.05f, 0.0f, 0.57f } };
    quad(scene, glass, s5, vec3(-0.2963993f, 0.0f, 0.9550642f));
    /* tall box (GGX metal): left, right, floor, ceiling, back, front */
    const float t0[4][3] = { { -0.53f, 0.0f, 0.09f }, { -0.53f, 1.2f, 0.09f }, { -0.71f, 1.2f, -0.49f }, { -0.71f, 0.0f, -0.49f } };
    quad(scene, metal, t0, vec3(-0.9550642f, 0.0f, 0.2963992f));
    const float t1[4][3] = { { -0.14f, 0.0f, -0.67f }, { -0.14f, 1.2f, -0.67f }, { 0.04f, 1.2f, -0.09f }, { 0.04f, 0.0f, -0.09f } };
    quad(scene, metal, t1, vec3(0.9550642f, 0.0f, -0.2963992f));
    const float t2[4][3] = { { -0.53f, 0.0f, 0.09f }, { 0.04f, 0.0f, -0.09f }, { -0.14f, 0.0f, -0.67f }, { -0.71f, 0.0f, -0.49f } };
    quad(scene, metal, t2, vec3(0.0f, -1.0f, 0.0f));
    const float t3[4][3] = { { -0.53f, 1.2f, 0.09f }, { 0.04f, 1.2f, -0.09f }, { -0.14f, 1.2f, -0.67f }, { -0.71f, 1.2f, -0.49f } };
    quad(scene, metal, t3, vec3(0.0f, 1.0f, 0.0f));
    const float t4[4][3] = { { -0.71f, 0.0f, -0.49f }, { -0.71f, 1.2f, -0.49f }, { -0.14f, 1.2f, -0.67f }, { -0.14f, 0.0f, -0.67f } };
    quad(scene, metal, t4, vec3(-0.3011314f, 0.0f, -0.9535826f));
    const float t5[4][3] = { { 0.04f, 0.0f, -0.09f }, { 0.04f, 1.2f, -0.09f }, { -0.53f, 1.2f, 0.09f }, { -0.53f, 0.0f, 0.09f } };
    quad(scene, metal, t5, vec3(0.3011314f, 0.0f, 0.9535826f));
    /* the light, the only hot spot */
    const float lamp[4][3] = { { -0.24f, 1.98f, 0.16f }, { -0.24f, 1.98f, -0.22f }, { 0.23f, 1.98f, -0.22f }, { 0.23f, 1.98f, 0.16f } };
    quad(scene, light, lamp, vec3(0.0f, -1.0f, 0.0f), HotSpot, { vec2(0.0f, 1.0f), vec2(0.0f, 0.0f), vec2(1.0f, 0.0f), vec2(1.0f, 1.0f) });
    scene.updateBVH();

    SensorRGBTransient sensor(width, height, start, sliceWidth, slices);
    Optics optics(Projection(radians(50.0f), sensor.aspectRatio()), LensDistortion(), LensDepthOfField(0.0f, 1.0f));
    Camera camera(optics, Transformation::fromLookAt(vec3(0.0f, 1.0f, 3.2f), vec3(0.0f, 1.0f, -1.0f), vec3(0.0f, 1.0f, 0.0f)));
    mcpt(sensor, camera, scene, samplesSqrt);

    bool ok = writePfm(outdir + "/frame.pfm", sensor.result());
    char name[32];
    for (unsigned int k = 0; k < sensor.binCount(); k++) {
        snprintf(name, sizeof(name), "/slice_%03u.pfm", k);
        ok = writePfm(outdir + name, sensor.bin(k)) && ok;
    }
    if (!ok) {
        fprintf(stderr, "light_in_flight: cannot write to %s\n", outdir.c_str());
        return 1;
    }
    printf("rendered %ux%u with %u spp and %u slices of path length %g from %g on kernel %s\n", width, height,
            samplesSqrt * samplesSqrt, sensor.binCount(), sliceWidth, start,
            sensor.bin(0).globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    return 0;
}
