/*
 * camera_rig.cpp -- a ring of cameras around a Cornell box, all rendered in ONE launch with the batch form of mcpt()
 * (include/wurblpt/wurblpt.hpp: mcpt(sensors, cameras, scene, ...)).  Small frames do not fill a GPU on their own; a batch of
 * views puts all their pixels into one launch.  Each view is bit for bit what mcpt() renders for its camera alone.  It links
 * libwurblpt_hip.so and nothing else; everything from mcpt() on runs on the GPU.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/camera_rig.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o camera_rig
 *   ./camera_rig [views width height samplesSqrt outdir]
 *
 * Writes view-000.png, view-001.png, ... (sRGB): the box seen from `views` points on an arc in front of its open side.
 */
#include <cmath>
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
    const unsigned int views = argc > 1 ? atoi(argv[1]) : 16;
    const unsigned int width = argc > 2 ? atoi(argv[2]) : 352;
    const unsigned int height = argc > 3 ? atoi(argv[3]) : 288;
    const unsigned int samplesSqrt = argc > 4 ? atoi(argv[4]) : 8;
    const std::string outdir = argc > 5 ? argv[5] : ".";

    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.725f, 0.71f, 0.68f)));
    Material* red = scene.take(new MaterialLambertian(vec3(0.63f, 0.065f, 0.05f)));
    Material* green = scene.take(new MaterialLambertian(vec3(0.14f, 0.45f, 0.091f)));
    Material* light = scene.take(new LightDiffuse(vec3(4.0f)));
    Material* metal = scene.take(new MaterialGGX(vec3(1.0f), vec2(0.04f)));
    quad(scene, red, vec3(-1, 0, 1), vec3(-1, 0, -1), vec3(-1, 2, -1), vec3(-1, 2, 1), vec3(1, 0, 0));
    quad(scene, green, vec3(1, 0, -1), vec3(1, 0, 1), vec3(1, 2, 1), vec3(1, 2, -1), vec3(-1, 0, 0));
    quad(scene, white, vec3(-1, 0, 1), vec3(1, 0, 1), vec3(1, 0, -1), vec3(-1, 0, -1), vec3(0, 1, 0));
    quad(scene, white, vec3(-1, 2, 1), vec3(-1, 2, -1), vec3(1, 2, -1), vec3(1, 2, 1), vec3(0, -1, 0));
    quad(scene, white, vec3(-1, 0, -1), vec3(1, 0, -1), vec3(1, 2, -1), vec3(-1, 2, -1), vec3(0, 0, 1));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(-0.4f, 0.4f, -0.3f), toQuat(radians(20.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f, 0.4f, 0.3f)))), metal));
    scene.take(new MeshInstance(scene.take(generateSphere(Transformation(vec3(0.45f, 0.3f, 0.3f), quat::null(), vec3(0.3f)))), white));
    quad(scene, light, vec3(-0.24f, 1.98f, 0.16f), vec3(-0.24f, 1.98f, -0.22f), vec3(0.23f, 1.98f, -0.22f), vec3(0.23f, 1.98f, 0.16f),
            vec3(0, -1, 0), HotSpot);
    scene.updateBVH();

    /* the rig: `views` cameras on an arc of +-50 degrees around the box's vertical axis, all aimed at its centre */
    std::vector<SensorRGB> sensorStore;
    sensorStore.reserve(views);
    std::vector<SensorRGB*> sensors;
    std::vector<Camera> cameras;
    const Optics optics(Projection(radians(50.0f), float(width) / height));
    for (unsigned int v = 0; v < views; v++) {
        const float a = radians(views > 1 ? -50.0f + 100.0f * v / (views - 1) : 0.0f);
        const vec3 eye(3.2f * std::sin(a), 1.0f, 3.2f * std::cos(a) - 0.2f);
        sensorStore.emplace_back(width, height);
        sensors.push_back(&sensorStore.back());
        cameras.emplace_back(optics, Transformation::fromLookAt(eye, vec3(0.0f, 1.0f, -0.2f), vec3(0.0f, 1.0f, 0.0f)));
    }
    mcpt(sensors, cameras, scene, samplesSqrt);

    std::string error;
    char name[64];
    for (unsigned int v = 0; v < views; v++) {
        const Array<float>& hdr = sensors[v]->result();
        snprintf(name, sizeof(name), "/view-%03u.png", v);
        if (!saveImage(toSRGB(uniformRationalQuantization(hdr, maxLuminance(hdr), 4.0f)), outdir + name, &error)) {
            fprintf(stderr, "%s\n", error.c_str());
            return 1;
        }
    }
    printf("rendered %u views of %ux%u with %u spp in one launch on kernel %s\n", views, width, height, samplesSqrt * samplesSqrt,
            sensors[0]->result().globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    return 0;
}
