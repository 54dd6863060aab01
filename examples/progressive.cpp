/*
 * progressive.cpp -- a Cornell box rendered in resumable stages (include/wurblpt/progressive.hpp: ProgressiveRender and mcpt()
 * with a callback per stage).  The frame is rendered k rows of strata at a time, and every stage leaves a preview to look at;
 * then the same frame is rendered again, stopped after its first stage, written to a checkpoint file, resumed from that file
 * and finished.  Both end with the frame of plain mcpt(), bit for bit, which the program checks.  It links libwurblpt_hip.so
 * and nothing else; everything from the first stage on runs on the GPU.
 *
 *   g++ -std=c++20 -O2 -fopenmp -Iinclude examples/progressive.cpp -Lwurblpt_amd/lib -lwurblpt_hip -Wl,-rpath,$PWD/wurblpt_amd/lib -o progressive
 *   ./progressive [width height samplesSqrt k outdir]
 *
 * Writes preview-RR.png after RR rows (sRGB), progressive.ckpt (the checkpoint), and the frames progressive.tgd,
 * progressive-resumed.tgd and plain.tgd (float arrays).  Exit status 1 if the three frames are not the same.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <wurblpt/wurblpt.hpp>
#include <wurblpt/progressive.hpp>

using namespace WurblPT;

static void quad(Scene& scene, const Material* m, const vec3& a, const vec3& b, const vec3& c, const vec3& d, const vec3& n,
        HotSpotType hot = ColdSpot)
{
    scene.take(new MeshInstance(scene.take(new Mesh({ a, b, c, d }, { n, n, n, n },
                        { vec2(0.0f, 0.0f), vec2(1.0f, 0.0f), vec2(1.0f, 1.0f), vec2(0.0f, 1.0f) }, { 0, 1, 2, 0, 2, 3 })), m), hot);
}

static bool same(const Array<float>& a, const Array<float>& b)
{
    return a.dataSize() == b.dataSize() && memcmp(a.data(), b.data(), a.dataSize()) == 0;
}

int main(int argc, char* argv[])
{
    const unsigned int width = argc > 1 ? atoi(argv[1]) : 512;
    const unsigned int height = argc > 2 ? atoi(argv[2]) : 512;
    const unsigned int samplesSqrt = argc > 3 ? atoi(argv[3]) : 16;
    const unsigned int k = argc > 4 && atoi(argv[4]) > 0 ? atoi(argv[4]) : 4;
    const std::string outdir = argc > 5 ? argv[5] : ".";

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
    std::string error;

    /* 1. in stages of k rows, a preview after each: the lower rows of every pixel's strata, so a picture, not an estimate */
    SensorRGB staged(width, height);
    bool written = true;
    mcpt(staged, camera, scene, samplesSqrt, 0.0f, 0.0f, Parameters(), [&](unsigned int rows, const Array<float>& preview) {
        char name[32];
        snprintf(name, sizeof(name), "/preview-%02u.png", rows);
        written = written && saveImage(toSRGB(uniformRationalQuantization(preview, maxLuminance(preview), 4.0f)), outdir + name, &error);
        printf("%u of %u rows of strata\n", rows, samplesSqrt);
        return written;
    }, k);

    /* 2. the first stage, a checkpoint, and the end of the session ... */
    SensorRGB resumed(width, height);
    const std::string checkpoint = outdir + "/progressive.ckpt";
    {
        ProgressiveRender first(resumed, camera, scene, samplesSqrt);
        first.advance(k);
        written = written && first.save(checkpoint, &error);
    }
    /* ... and, as another run of the program would, the rest from the file */
    if (written) {
        ProgressiveRender rest = ProgressiveRender::resume(checkpoint, resumed, camera, scene);
        printf("resumed at %u of %u rows of strata\n", rest.rowsDone(), rest.rowsTotal());
        while (!rest.finished())
            rest.advance(k);
    }

    /* 3. the frame in one piece */
    SensorRGB plain(width, height);
    mcpt(plain, camera, scene, samplesSqrt);

    if (!written || !saveImage(staged.result(), outdir + "/progressive.tgd", &error)
            || !saveImage(resumed.result(), outdir + "/progressive-resumed.tgd", &error)
            || !saveImage(plain.result(), outdir + "/plain.tgd", &error)) {
        fprintf(stderr, "%s\n", error.c_str());
        return 1;
    }
    const bool identical = same(staged.result(), plain.result()) && same(resumed.result(), plain.result());
    printf("rendered %ux%u with %u samples in stages of %u rows on kernel %s: staged and resumed frames %s the frame of mcpt()\n", width, height,
            samplesSqrt * samplesSqrt, k, staged.result().globalTagList().value("WURBLPT/DEVICE_KERNEL").c_str(),
            identical ? "are bit for bit" : "DIFFER from");
    return identical ? 0 : 1;
}
