/*
 * tof_camera.cpp -- a first program for the time-of-flight camera (include/wurblpt/tof.hpp): the room of the reference's
 * wurblpt-tof-example application at rest (a white wall two metres away, a glossy quad and an icosahedron in front of it) with
 * a ToF light at the camera.  The four phase images of one exposure are rendered in ONE launch -- a pixel's paths do not
 * depend on the phase, so the reference's four renders trace the same paths four times -- and SensorTofAmcw::result() turns
 * them into distances.  Prints the distance the camera measures in the centre pixel beside the ground truth.  It links
 * libwurblpt_hip.so and nothing else; everything from mcpt() on runs on the GPU.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/tof_camera.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o tof_camera
 *   ./tof_camera [width height samplesSqrt outdir maxPathComponents]
 *
 * Writes energies-J.pfm (a, b, total of phase image J; rows bottom-up like the sensor) and result.pfm (distance, amplitude,
 * intensity).
 */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <wurblpt/wurblpt.hpp>
#include <wurblpt/tof.hpp>

using namespace WurblPT;

static bool writePfm(const std::string& name, const Array<float>& a)
{
    FILE* f = fopen(name.c_str(), "wb");
    if (!f)
        return false;
    fprintf(f, "PF\n%zu %zu\n-1.0\n", a.dimension(0), a.dimension(1));
    bool ok = true;
    for (size_t i = 0; i < a.elementCount() && ok; i++)
        ok = fwrite(a[i], sizeof(float), 3, f) == 3; /* the first three components */
    return fclose(f) == 0 && ok;
}

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 352;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 288;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 10;
    const std::string outdir = argc > 4 ? argv[4] : ".";
    const unsigned int maxPathComponents = argc > 5 ? atoi(argv[5]) : 2; /* 2: only direct illumination */

    Scene scene;
    Material* bgMaterial = scene.take(new MaterialLambertian(vec4(1.0f)));
    Transformation bgTransformation(vec3(0.0f, 0.0f, -2.0f), quat::null(), vec3(5.0f));
    scene.take(new MeshInstance(scene.take(generateQuad(bgTransformation)), bgMaterial));
    Material* quadMaterial = scene.take(new MaterialModPhong(vec3(0.7f), vec3(0.3f), 100.0f));
    Transformation quadTransformation(vec3(0.0f), quat::null(), vec3(0.2f));
    scene.take(new MeshInstance(scene.take(generateQuad(quadTransformation)), quadMaterial, Transformation(vec3(-1.0f, 0.5f, -1.5f))));
    Material* objectMaterial = scene.take(new MaterialModPhong(vec3(0.5f), vec3(0.5f), 100.0f));
    Transformation objectTransformation(vec3(0.0f), quat::null(), vec3(0.33f));
    scene.take(new MeshInstance(scene.take(generateIcosahedron(objectTransformation)), objectMaterial,
                Transformation(vec3(0.0f, -0.3f, -1.0f), toQuat(radians(0.0f), vec3(0.0f, 1.0f, 0.5f)))));
    /* the light sits at the camera and looks where it looks; its back side is black */
    Material* lightFrontSide = scene.take(new LightTof(40.0f / (4.0f * pi), radians(120.0f)));
    Material* lightBackSide = scene.take(new MaterialLambertian(vec4(0.0f)));
    Material* lightMaterial = scene.take(new MaterialTwoSided(lightFrontSide, lightBackSide));
    Transformation lightTransformation(vec3(0.0f), toQuat(radians(180.0f), vec3(1.0f, 0.0f, 0.0f)), vec3(0.10f, 0.05f, 1.0f));
    scene.take(new MeshInstance(scene.take(generateQuad(lightTransformation)), lightMaterial), HotSpot);
    scene.updateBVH();

    SensorTofAmcw sensor(width, height);
    Camera camera(Optics(Projection(radians(70.0f), sensor.aspectRatio())));
    Parameters params;
    params.maxPathComponents = maxPathComponents;
    params.rrThreshold = 0.0f;

    std::vector<Array<float>> energies;
    mcpt(energies, sensor, camera, scene, samplesSqrt, 0.0f, 0.0f, params); /* all sensor.phaseImageCount phase images */
    std::vector<Array<float>> phases;
    for (const Array<float>& e : energies)
        phases.push_back(sensor.phase(e, 0.0f)); /* no shot noise */
    const Array<float> result = sensor.result(phases.data());
    const GroundTruth gt = getGroundTruth(sensor, camera, scene, 0.0f, GroundTruth::CameraSpaceDistances);

    bool ok = writePfm(outdir + "/result.pfm", result);
    for (size_t j = 0; j < energies.size(); j++)
        ok = writePfm(outdir + "/energies-" + std::to_string(j) + ".pfm", energies[j]) && ok;
    if (!ok) {
        fprintf(stderr, "tof_camera: cannot write to %s\n", outdir.c_str());
        return 1;
    }
    const unsigned int cx = width / 2, cy = height / 2;
    printf("rendered %zu phase images of %ux%u with %u spp in one launch on kernel %s\n", energies.size(), width, height,
            samplesSqrt * samplesSqrt, energies[0].globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    printf("centre pixel: measured distance %.4f m, ground truth %.4f m\n", result.at(cx, cy)[0], gt.cameraSpaceDistances.at(cx, cy)[0]);
    return 0;
}
