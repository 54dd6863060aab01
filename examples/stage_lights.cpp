/*
 * stage_lights.cpp -- spot lights (LightSpot) on a small stage, written against include/wurblpt the way the reference's
 * wurblpt-stagelights application is written against libwurblpt.  Three lamps hang 2.4 above a white floor and point
 * straight down: a red one, a blue one and a white one whose emission is a checker texture.  Each lights a round pool on
 * the floor; the back curtain is black, so the floor outside every cone gets no light at all.  It links
 * libwurblpt_hip.so and nothing else; everything from mcpt() on runs on the GPU.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/stage_lights.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o stage_lights
 *   ./stage_lights [width height samplesSqrt outdir]
 *
 * Writes stage.png (sRGB), stage.pfm (the linear frame) and stage-positions.pfm (world space positions from
 * getGroundTruth).
 */
#include <cstdio>
#include <cstdlib>
#include <string>

#include <wurblpt/wurblpt.hpp>

using namespace WurblPT;

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 640;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 360;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 8;
    const std::string outdir = argc > 4 ? argv[4] : ".";

    Scene scene;
    Material* floor = scene.take(new MaterialLambertian(vec3(0.75f)), "floor");
    Material* curtain = scene.take(new MaterialLambertian(vec3(0.0f)), "curtain");
    Texture* gobo = scene.take(new TextureChecker(vec3(1.0f), vec3(0.05f), 4, 4));
    /* LightSpot(openingAngle, emission [, emission texture]): the full angle of the cone around the lamp's normal */
    Material* red = scene.take(new LightSpot(radians(30.0f), vec3(10.0f, 1.5f, 1.0f)), "red spot");
    Material* blue = scene.take(new LightSpot(radians(24.0f), vec3(1.0f, 2.0f, 12.0f)), "blue spot");
    Material* patterned = scene.take(new LightSpot(radians(36.0f), vec3(8.0f), gobo), "patterned spot");

    /* generateQuad() makes a quad in the xy plane, [-1,1]^2, facing +z */
    const quat toFloor = toQuat(radians(-90.0f), vec3(1.0f, 0.0f, 0.0f));
    const quat down = toQuat(radians(90.0f), vec3(1.0f, 0.0f, 0.0f));
    scene.take(new MeshInstance(scene.take(generateQuad()), floor, Transformation(vec3(0.0f), toFloor, vec3(3.0f, 2.0f, 1.0f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), curtain, Transformation(vec3(0.0f, 1.5f, -2.0f), quat::null(), vec3(3.0f, 1.5f, 1.0f))));
    /* the lamps, 0.3 x 0.3, all hot spots */
    scene.take(new MeshInstance(scene.take(generateQuad()), red, Transformation(vec3(-1.5f, 2.4f, 0.0f), down, vec3(0.15f))), HotSpot);
    scene.take(new MeshInstance(scene.take(generateQuad()), blue, Transformation(vec3(0.0f, 2.4f, -0.6f), down, vec3(0.15f))), HotSpot);
    scene.take(new MeshInstance(scene.take(generateQuad()), patterned, Transformation(vec3(1.5f, 2.4f, 0.2f), down, vec3(0.15f))), HotSpot);

    Optics optics(Projection(radians(45.0f), float(width) / height));
    Camera camera(optics, Transformation::fromLookAt(vec3(0.0f, 2.0f, 5.5f), vec3(0.0f, 0.6f, 0.0f)));
    std::string error;

    scene.updateBVH();
    SensorRGB sensor(width, height);
    mcpt(sensor, camera, scene, samplesSqrt);
    const Array<float>& hdr = sensor.result();
    if (!saveImage(hdr, outdir + "/stage.pfm", &error) || !saveImage(toSRGB(uniformRationalQuantization(hdr, maxLuminance(hdr) / 20.0f, 8.0f)), outdir + "/stage.png", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    GroundTruth gt = getGroundTruth(sensor, camera, scene, 0.0f, GroundTruth::WorldSpacePositions);
    if (!saveImage(gt.worldSpacePositions, outdir + "/stage-positions.pfm", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    fprintf(stderr, "%s\n", hdr.globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str());
    return 0;
}
