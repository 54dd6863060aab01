/*
 * denoise_textured.cpp -- a room whose walls and floor carry checker textures, at 16 samples per pixel, filtered twice: as
 * radiance (denoise(), which takes the checker's contrast for noise wherever it lies within the luminance tolerance) and
 * demodulated (the overload of denoise() that takes albedo and emission, include/wurblpt/postproc.hpp): getFirstHitColours()
 * says per pixel what the surface multiplies the light with and what it emits itself, the filter runs on (frame - emission) /
 * albedo, and the colours are put back afterwards (include/wurblpt_hip.h has the rule).  The same call gives the filter's guide,
 * so no getGroundTruth() is needed.  It links libwurblpt_hip.so and nothing else; the render and the first-hit pass run on the
 * GPU, the filters here on the CPU with the bits of the device's entry points.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/denoise_textured.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o denoise_textured
 *   ./denoise_textured [width height samplesSqrt iterations outdir]
 *
 * Writes textured-noisy.png, textured-denoised.png and textured-demodulated.png (sRGB, one tone mapping for all).
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
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 4;
    DenoiseParameters params;
    if (argc > 4)
        params.iterations = atoi(argv[4]);
    const std::string outdir = argc > 5 ? argv[5] : ".";

    Scene scene;
    Texture* tiles = scene.take(new TextureChecker(vec3(0.75f, 0.72f, 0.65f), vec3(0.25f, 0.12f, 0.08f), 12, 12));
    Texture* paper = scene.take(new TextureChecker(vec3(0.2f, 0.3f, 0.7f), vec3(0.85f), 16, 16));
    Material* floor = scene.take(new MaterialLambertian(vec3(0.5f), tiles));
    Material* wall = scene.take(new MaterialLambertian(vec3(0.5f), paper));
    Material* white = scene.take(new MaterialLambertian(vec3(0.725f, 0.71f, 0.68f)));
    Material* light = scene.take(new LightDiffuse(vec3(4.0f)));
    quad(scene, wall, vec3(-1, 0, 1), vec3(-1, 0, -1), vec3(-1, 2, -1), vec3(-1, 2, 1), vec3(1, 0, 0));
    quad(scene, wall, vec3(1, 0, -1), vec3(1, 0, 1), vec3(1, 2, 1), vec3(1, 2, -1), vec3(-1, 0, 0));
    quad(scene, floor, vec3(-1, 0, 1), vec3(1, 0, 1), vec3(1, 0, -1), vec3(-1, 0, -1), vec3(0, 1, 0));
    quad(scene, white, vec3(-1, 2, 1), vec3(-1, 2, -1), vec3(1, 2, -1), vec3(1, 2, 1), vec3(0, -1, 0));
    quad(scene, wall, vec3(-1, 0, -1), vec3(1, 0, -1), vec3(1, 2, -1), vec3(-1, 2, -1), vec3(0, 0, 1));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(-0.35f, 0.6f, -0.3f), toQuat(radians(20.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f, 0.6f, 0.3f)))), white));
    quad(scene, light, vec3(-0.24f, 1.98f, 0.16f), vec3(-0.24f, 1.98f, -0.22f), vec3(0.23f, 1.98f, -0.22f), vec3(0.23f, 1.98f, 0.16f),
            vec3(0, -1, 0), HotSpot);
    scene.updateBVH();
    const Camera camera(Optics(Projection(radians(50.0f), float(width) / height)),
            Transformation::fromLookAt(vec3(0.0f, 1.0f, 3.2f), vec3(0.0f, 1.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f)));

    /* 1. the frame and its moment film: every pixel at samplesSqrt^2 samples */
    SensorRGB sensor(width, height);
    Array<float> moments;
    mcpt(sensor, camera, scene, std::vector<uint16_t>(size_t(width) * height, uint16_t(samplesSqrt)), 0.0f, 0.0f, Parameters(), &moments);
    /* 2. what the ray through each pixel's centre hits first: the surface's colours and the filter's guide, from one walk */
    const FirstHitColours fh = getFirstHitColours(sensor, camera, scene);
    /* 3. the filter, on the radiance and on the demodulated frame */
    const Array<float>& noisy = sensor.result();
    const Array<float> denoised = denoise(noisy, moments, samplesSqrt, fh.cameraSpacePositions, fh.cameraSpaceMaterialNormals, fh.materials, params);
    const Array<float> demodulated = denoise(noisy, moments, samplesSqrt, fh.cameraSpacePositions, fh.cameraSpaceMaterialNormals, fh.materials,
            fh.albedo, fh.emission, params);

    const float maxLum = maxLuminance(demodulated) / 800.0f;
    std::string error;
    if (!saveImage(toSRGB(uniformRationalQuantization(noisy, maxLum, 4.0f)), outdir + "/textured-noisy.png", &error)
            || !saveImage(toSRGB(uniformRationalQuantization(denoised, maxLum, 4.0f)), outdir + "/textured-denoised.png", &error)
            || !saveImage(toSRGB(uniformRationalQuantization(demodulated, maxLum, 4.0f)), outdir + "/textured-demodulated.png", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    printf("rendered %ux%u at %u spp on kernel %s and filtered it with %u iterations: textured-noisy.png, textured-denoised.png, textured-demodulated.png\n",
            width, height, samplesSqrt * samplesSqrt, noisy.globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str(), params.iterations);
    return 0;
}
