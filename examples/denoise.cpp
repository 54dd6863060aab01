/*
 * denoise.cpp -- a Cornell box at 16 samples per pixel, and the same frame after the denoiser (include/wurblpt/postproc.hpp:
 * denoise()).  The frame is rendered through the adaptive entry point (mcpt() with a sample-count map), which also fills the
 * moment film the filter takes its variance estimate from; getGroundTruth() gives the noise-free guide (camera space positions
 * and material normals, material indices); denoise() is the edge-avoiding a-trous wavelet filter with variance guidance
 * (include/wurblpt_hip.h has the formula).  It links libwurblpt_hip.so and nothing else; the render and the first-hit pass run
 * on the GPU, the filter here on the CPU with the bits of the device's wpt_postproc_denoise.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/denoise.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o denoise
 *   ./denoise [width height samplesSqrt iterations outdir]
 *
 * Writes noisy.png, denoised.png and despeckled.png (sRGB, one tone mapping for all): the last is the noisy frame after
 * despeckle(), the 3 x 3 firefly filter, which takes single outliers out and leaves the noise.
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
    Material* white = scene.take(new MaterialLambertian(vec3(0.725f, 0.71f, 0.68f)));
    Material* red = scene.take(new MaterialLambertian(vec3(0.63f, 0.065f, 0.05f)));
    Material* green = scene.take(new MaterialLambertian(vec3(0.14f, 0.45f, 0.091f)));
    Material* light = scene.take(new LightDiffuse(vec3(4.0f)));
    quad(scene, red, vec3(-1, 0, 1), vec3(-1, 0, -1), vec3(-1, 2, -1), vec3(-1, 2, 1), vec3(1, 0, 0));
    quad(scene, green, vec3(1, 0, -1), vec3(1, 0, 1), vec3(1, 2, 1), vec3(1, 2, -1), vec3(-1, 0, 0));
    quad(scene, white, vec3(-1, 0, 1), vec3(1, 0, 1), vec3(1, 0, -1), vec3(-1, 0, -1), vec3(0, 1, 0));
    quad(scene, white, vec3(-1, 2, 1), vec3(-1, 2, -1), vec3(1, 2, -1), vec3(1, 2, 1), vec3(0, -1, 0));
    quad(scene, white, vec3(-1, 0, -1), vec3(1, 0, -1), vec3(1, 2, -1), vec3(-1, 2, -1), vec3(0, 0, 1));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(-0.35f, 0.6f, -0.3f), toQuat(radians(20.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f, 0.6f, 0.3f)))), white));
    scene.take(new MeshInstance(scene.take(generateCube(Transformation(vec3(0.4f, 0.3f, 0.3f), toQuat(radians(-17.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f)))), white));
    quad(scene, light, vec3(-0.24f, 1.98f, 0.16f), vec3(-0.24f, 1.98f, -0.22f), vec3(0.23f, 1.98f, -0.22f), vec3(0.23f, 1.98f, 0.16f),
            vec3(0, -1, 0), HotSpot);
    scene.updateBVH();
    const Camera camera(Optics(Projection(radians(50.0f), float(width) / height)),
            Transformation::fromLookAt(vec3(0.0f, 1.0f, 3.2f), vec3(0.0f, 1.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f)));

    /* 1. the frame and its moment film: every pixel at samplesSqrt^2 samples */
    SensorRGB sensor(width, height);
    Array<float> moments;
    mcpt(sensor, camera, scene, std::vector<uint16_t>(size_t(width) * height, uint16_t(samplesSqrt)), 0.0f, 0.0f, Parameters(), &moments);
    /* 2. the guide: what the ray through each pixel's centre hits first */
    const GroundTruth gt = getGroundTruth(sensor, camera, scene, 0.0f,
            GroundTruth::CameraSpacePositions | GroundTruth::CameraSpaceMaterialNormals | GroundTruth::Materials);
    /* 3. the filter */
    const Array<float>& noisy = sensor.result();
    const Array<float> denoised = denoise(noisy, moments, samplesSqrt, gt.cameraSpacePositions, gt.cameraSpaceMaterialNormals, gt.materials, params);

    /* white at an eighth of the lamp's luminance (maxLuminance() is Y * 100): the walls, where the noise is, fill the range */
    const float maxLum = maxLuminance(denoised) / 800.0f;
    std::string error;
    if (!saveImage(toSRGB(uniformRationalQuantization(noisy, maxLum, 4.0f)), outdir + "/noisy.png", &error)
            || !saveImage(toSRGB(uniformRationalQuantization(despeckle(noisy), maxLum, 4.0f)), outdir + "/despeckled.png", &error)
            || !saveImage(toSRGB(uniformRationalQuantization(denoised, maxLum, 4.0f)), outdir + "/denoised.png", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    printf("rendered %ux%u at %u spp on kernel %s and filtered it with %u iterations: noisy.png, denoised.png, despeckled.png\n", width, height,
            samplesSqrt * samplesSqrt, noisy.globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str(), params.iterations);
    return 0;
}
