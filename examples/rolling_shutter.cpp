/*
 * rolling_shutter.cpp -- what a CMOS sensor delivers that a global shutter does not: a camera pans past upright bars while a
 * blade turns on the back wall.  The first picture exposes the whole frame at one instant (mcpt); the second reads the rows
 * from the top, one after the other, each at its own instant (mcptRollingShutter, include/wurblpt/shutter.hpp): the bars lean
 * and the blade bends.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/rolling_shutter.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o rolling_shutter
 *   ./rolling_shutter [width height samplesSqrt outdir]
 *
 * Writes global-shutter.png and rolling-shutter.png.  The row read first is exposed at the global shutter's instant, so it
 * must be that picture's row bit for bit; the program exits with 1 if it is not (and with 2 if no other row differs: then
 * nothing rolled).
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <wurblpt/wurblpt.hpp>
#include <wurblpt/shutter.hpp>

using namespace WurblPT;

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 640;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 480;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 6;
    const std::string outdir = argc > 4 ? argv[4] : ".";

    Scene scene;
    Material* white = scene.take(new MaterialLambertian(vec3(0.73f)), "white");
    Material* blue = scene.take(new MaterialLambertian(vec3(0.15f, 0.25f, 0.65f)), "blue");
    Material* orange = scene.take(new MaterialLambertian(vec3(0.8f, 0.4f, 0.1f)), "orange");
    Material* lamp = scene.take(new LightDiffuse(vec3(10.0f)), "lamp");

    /* a wide room, open towards the camera */
    const quat toFloor = toQuat(radians(-90.0f), vec3(1.0f, 0.0f, 0.0f));
    const quat toCeiling = toQuat(radians(90.0f), vec3(1.0f, 0.0f, 0.0f));
    scene.take(new MeshInstance(scene.take(generateQuad()), white, Transformation(vec3(0.0f, 0.0f, 0.0f), toFloor, vec3(3.0f, 1.5f, 1.0f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), white, Transformation(vec3(0.0f, 2.0f, 0.0f), toCeiling, vec3(3.0f, 1.5f, 1.0f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), white, Transformation(vec3(0.0f, 1.0f, -1.5f), quat::null(), vec3(3.0f, 1.0f, 1.0f))));
    scene.take(new MeshInstance(scene.take(generateQuad()), lamp, Transformation(vec3(0.0f, 1.99f, 0.3f), toCeiling, vec3(1.2f, 0.4f, 1.0f))), HotSpot);
    /* upright bars */
    for (int i = -3; i <= 3; i++)
        scene.take(new MeshInstance(scene.take(generateCube()), blue, Transformation(vec3(0.5f * i, 1.0f, 0.0f), quat::null(), vec3(0.04f, 1.0f, 0.04f))));
    /* a blade on the back wall: one turn per second about the z axis */
    std::vector<AnimationKeyframes::Keyframe> turn;
    for (int k = 0; k <= 8; k++)
        turn.emplace_back(0.125f * k, Transformation(vec3(0.0f, 1.0f, -1.2f), toQuat(radians(45.0f * k), vec3(0.0f, 0.0f, 1.0f)), vec3(0.06f, 0.8f, 1.0f)));
    const int turning = scene.take(new AnimationKeyframes(turn));
    scene.take(new MeshInstance(scene.take(generateQuad()), orange, turning));

    /* the camera pans from left to right between t = 0 and t = 1 */
    const Optics optics(Projection(radians(45.0f), float(width) / height));
    const Camera camera(optics, new AnimationKeyframes(0.0f, Transformation::fromLookAt(vec3(-0.6f, 1.0f, 3.4f), vec3(-0.6f, 1.0f, 0.0f)),
                1.0f, Transformation::fromLookAt(vec3(0.6f, 1.0f, 3.4f), vec3(0.6f, 1.0f, 0.0f))));

    /* both pictures start at t = 0.25; the rolling one takes half a second to read its rows, top row first, each an instant */
    const float t = 0.25f;
    RollingShutter shutter;
    shutter.rowTime = 0.5f / height;
    shutter.fromTop = true;
    /* the scene bounded for the whole readout serves both renders */
    scene.updateBVH(t, shutter.end(t, t, height));

    SensorRGB global(width, height), rolling(width, height);
    mcpt(global, camera, scene, samplesSqrt, t, t);
    mcptRollingShutter(rolling, camera, scene, samplesSqrt, t, t, shutter);

    std::string error;
    const float white_point = maxLuminance(global.result()) / 100.0f;
    if (!saveImage(toSRGB(uniformRationalQuantization(global.result(), white_point, 8.0f)), outdir + "/global-shutter.png", &error)
            || !saveImage(toSRGB(uniformRationalQuantization(rolling.result(), white_point, 8.0f)), outdir + "/rolling-shutter.png", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 3;
    }

    /* frames are stored bottom row first: the row read first is the last one in memory */
    const float* g = static_cast<const float*>(global.result().data());
    const float* r = static_cast<const float*>(rolling.result().data());
    const size_t rowFloats = size_t(width) * 3;
    unsigned int differing = 0;
    for (unsigned int y = 0; y + 1 < height; y++)
        differing += memcmp(g + y * rowFloats, r + y * rowFloats, rowFloats * sizeof(float)) != 0 ? 1 : 0;
    const bool firstRowEqual = memcmp(g + (height - 1) * rowFloats, r + (height - 1) * rowFloats, rowFloats * sizeof(float)) == 0;
    fprintf(stderr, "row read first %s the global shutter's; %u of the other %u rows differ from it\n", firstRowEqual ? "equals" : "DIFFERS from",
            differing, height - 1);
    if (!firstRowEqual)
        return 1;
    return differing > 0 ? 0 : 2;
}
