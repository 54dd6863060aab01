/*
 * wurblpt.hpp -- the public entry point: Parameters and mcpt() with the reference's
 * signatures (wurblpt.hpp:79-96,279-286,439-449).
 *
 * mcpt() does what the reference's does -- renders samplesSqrt^2 samples per pixel into the
 * sensor's frame -- by flattening the scene and handing pixel blocks to the MI355X kernels
 * behind the C ABI of include/wurblpt_hip.h.  There is no CPU fallback: without a device, or
 * with scene content the kernels do not know, it prints the reason and aborts (the reference's
 * own fatal-error behaviour, bvh.hpp:260-263).
 */
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../wurblpt_hip.h"
#include "animation.hpp"
#include "camera.hpp"
#include "constants.hpp"
#include "envmap.hpp"
#include "generator.hpp"
#include "gvm.hpp"
#include "imageio.hpp"
#include "import.hpp"
#include "material.hpp"
#include "mesh.hpp"
#include "mpi.hpp"
#include "postproc.hpp"
#include "prng.hpp"
#include "scene.hpp"
#include "sensor.hpp"
#include "texture.hpp"
#include "transformation.hpp"

namespace WurblPT {

class Parameters
{
public:
    unsigned int maxPathComponents;
    float rrThreshold;
    bool randomizeRayOverPixel;
    float minHitDistance;

    Parameters() : maxPathComponents(128), rrThreshold(1.0f), randomizeRayOverPixel(true), minHitDistance(0.00001f) {}
};

inline wpt_params makeParams(const Parameters& params, const SensorRGB& sensor)
{
    wpt_params p;
    p.max_path_components = params.maxPathComponents;
    p.rr_threshold = params.rrThreshold;
    p.randomize_ray_over_pixel = params.randomizeRayOverPixel ? 1 : 0;
    p.min_hit_distance = params.minHitDistance;
    p.min_dist_to_light = sensor.minDistToLight;
    p.max_dist_to_light = sensor.maxDistToLight;
    p.min_path_len = sensor.minPathLen;
    p.max_path_len = sensor.maxPathLen;
    p.t0 = 0.0f;
    p.t1 = 0.0f;
    return p;
}

[[noreturn]] inline void mcptFatal(const std::string& what)
{
    fprintf(stderr, "mcpt: %s\n", what.c_str());
    abort();
}

inline void mcptTransient(MPICoordinator& mpiCoordinator, SensorRGBTransient& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0, float t1, const Parameters& params);

inline void mcptLightGroups(MPICoordinator& mpiCoordinator, SensorRGBLightGroups& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0, float t1, const Parameters& params);

inline void mcpt(MPICoordinator& mpiCoordinator, Sensor& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0 = 0.0f, float t1 = 0.0f, const Parameters& params = Parameters())
{
    if (scene.bvhNeedsUpdate(t0, t1))
        mcptFatal("Scene::updateBVH(t0, t1) must run before mcpt()");
    if (SensorRGBLightGroups* groups = dynamic_cast<SensorRGBLightGroups*>(&sensor)) {
        mcptLightGroups(mpiCoordinator, *groups, camera, scene, samplesSqrt, t0, t1, params);
        return;
    }
    if (SensorRGBTransient* transient = dynamic_cast<SensorRGBTransient*>(&sensor)) {
        mcptTransient(mpiCoordinator, *transient, camera, scene, samplesSqrt, t0, t1, params);
        return;
    }
    SensorRGB* rgb = dynamic_cast<SensorRGB*>(&sensor);
    if (!rgb)
        mcptFatal("only SensorRGB runs on the device path");
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    if (camera.animation) {
        /* the camera's key frames join the scene's pool; rays take them at their own time when t0 != t1 */
        cam.animation = flat.addAnimation(camera.animation.get());
        if (cam.animation < 0)
            mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
    }
    const wpt_scene_desc desc = flat.desc();
    wpt_params p = makeParams(params, *rgb);
    p.t0 = t0;
    p.t1 = t1;
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    ArrayContainer* pixelArray = sensor.pixelArray();

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples.\n", width, height, samplesSqrt * samplesSqrt);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());

    mpiCoordinator.init(width, height, static_cast<float*>(pixelArray->data()), pixelArray->componentCount());
    std::vector<std::string> workerErrors(mpiCoordinator.devices().size());
    const auto renderStart = std::chrono::steady_clock::now();
    auto worker = [&](size_t w) {
        int device = mpiCoordinator.devices()[w];
        if (device >= 0 && wpt_select_device(device) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        wpt_scene* dscene = nullptr;
        if (wpt_scene_upload(&desc, &dscene) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        if (mpiCoordinator.devices().size() > 1) {
            /* several devices: a lane owns a pixel for all its samples, so a device is only as busy as it has pixels in
             * flight.  Each device takes its share in ONE launch -- the bands of 16 rows whose index is w modulo the number
             * of devices -- and writes them into the shared frame (wurblpt_hip.h: wpt_render_bands). */
            const unsigned int count = mpiCoordinator.devices().size();
            fprintf(stderr, "%s: device %d renders bands %zu, %zu, ... of 16 rows\n", mpiCoordinator.processId(), device, w, w + count);
            if (wpt_render_bands(dscene, &cam, &p, width, height, samplesSqrt, 16, w, count, mpiCoordinator.blockData(0)) != WPT_OK)
                workerErrors[w] = wpt_last_error();
            wpt_scene_free(dscene);
            return;
        }
        for (;;) {
            unsigned int blockStart, blockSize;
            mpiCoordinator.getBlock(&blockStart, &blockSize);
            if (blockSize == 0)
                break;
            fprintf(stderr, "%s: device %d renders block of size %u starting at %u\n", mpiCoordinator.processId(), device, blockSize, blockStart);
            if (wpt_render_block(dscene, &cam, &p, width, height, samplesSqrt, blockStart, blockSize,
                        mpiCoordinator.blockData(blockStart)) != WPT_OK) {
                workerErrors[w] = wpt_last_error();
                break;
            }
            mpiCoordinator.submitBlock(blockStart, blockSize);
        }
        wpt_scene_free(dscene);
    };
    if (mpiCoordinator.devices().size() == 1) {
        worker(0);
    } else {
        std::vector<std::thread> threads;
        for (size_t w = 0; w < mpiCoordinator.devices().size(); w++)
            threads.emplace_back(worker, w);
        for (auto& t : threads)
            t.join();
    }
    mpiCoordinator.finish();
    for (const std::string& e : workerErrors)
        if (!e.empty())
            mcptFatal(e);

    pixelArray->globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(samplesSqrt * samplesSqrt));
    pixelArray->globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
    pixelArray->globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
    pixelArray->globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
    /* the run's record (wurblpt.hpp:393-400,425-435 notes compiler, CPU model, threads and CPU seconds): here the
     * compiler of the kernels, the device(s) and the wall-clock seconds from scene upload to the finished frame */
    std::string deviceModel;
    for (int device : mpiCoordinator.devices()) {
        int current = device;
        if (current < 0 && wpt_current_device(&current) != WPT_OK)
            current = 0;
        deviceModel += (deviceModel.empty() ? "" : "; ") + std::string(wpt_device_name(current));
    }
    pixelArray->globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
    pixelArray->globalTagList().set("WURBLPT/DEVICE_MODEL", deviceModel);
    pixelArray->globalTagList().set("WURBLPT/DEVICE_COUNT", std::to_string(mpiCoordinator.devices().size()));
    pixelArray->globalTagList().set("WURBLPT/DEVICE_SECONDS",
            std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count()));
}

/* mcpt() for a batch of views: sensor i is rendered from camera i, all of them in one launch on one device (wurblpt_hip.h:
 * wpt_render_views).  Each sensor's frame is bit for bit what mcpt(sensor, camera i, ...) writes, and carries the same tags.
 * One wpt_params serves the batch, so the sensors must agree in size and in their four gates; that, and one sensor per camera,
 * is checked before any device work (std::invalid_argument).  Several devices and MPI ranks are not served. */
inline void mcpt(const std::vector<SensorRGB*>& sensors, const std::vector<Camera>& cameras, const Scene& scene,
        unsigned int samplesSqrt, float t0 = 0.0f, float t1 = 0.0f, const Parameters& params = Parameters())
{
    if (sensors.empty() || sensors.size() != cameras.size())
        throw std::invalid_argument("mcpt: a batch of views needs one sensor per camera, and at least one of each");
    for (const SensorRGB* s : sensors) {
        if (!s)
            throw std::invalid_argument("mcpt: a sensor of the batch is NULL");
        const SensorRGB& s0 = *sensors[0];
        if (s->width() != s0.width() || s->height() != s0.height())
            throw std::invalid_argument("mcpt: the sensors of a batch of views must have one size");
        if (s->minDistToLight != s0.minDistToLight || s->maxDistToLight != s0.maxDistToLight || s->minPathLen != s0.minPathLen
                || s->maxPathLen != s0.maxPathLen)
            throw std::invalid_argument("mcpt: the sensors of a batch of views must have the same distance and path length gates");
    }
    if (scene.bvhNeedsUpdate(t0, t1))
        mcptFatal("Scene::updateBVH(t0, t1) must run before mcpt()");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    const uint32_t viewCount = uint32_t(cameras.size());
    std::vector<wpt_camera> cams(viewCount);
    for (uint32_t v = 0; v < viewCount; v++) {
        if (!cameras[v].describe(cams[v], t0))
            mcptFatal("this camera cannot be described to the device path");
        if (cameras[v].animation) {
            /* each camera's key frames join the scene's pool */
            cams[v].animation = flat.addAnimation(cameras[v].animation.get());
            if (cams[v].animation < 0)
                mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
        }
    }
    const wpt_scene_desc desc = flat.desc();
    wpt_params p = makeParams(params, *sensors[0]);
    p.t0 = t0;
    p.t1 = t1;
    const unsigned int width = sensors[0]->width();
    const unsigned int height = sensors[0]->height();

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %u views of %ux%u pixels with %u samples.\n", viewCount, width, height, samplesSqrt * samplesSqrt);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());
    const auto renderStart = std::chrono::steady_clock::now();
    wpt_scene* dscene = nullptr;
    if (wpt_scene_upload(&desc, &dscene) != WPT_OK)
        mcptFatal(wpt_last_error());
    const size_t frameFloats = size_t(width) * height * 3;
    std::vector<float> frames(frameFloats * viewCount);
    const wpt_status st = wpt_render_views(dscene, cams.data(), viewCount, &p, width, height, samplesSqrt, frames.data());
    wpt_scene_free(dscene);
    if (st != WPT_OK)
        mcptFatal(wpt_last_error());

    int device = 0;
    if (wpt_current_device(&device) != WPT_OK)
        device = 0;
    const std::string seconds = std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count());
    for (uint32_t v = 0; v < viewCount; v++) {
        ArrayContainer* a = sensors[v]->pixelArray();
        std::copy(frames.begin() + v * frameFloats, frames.begin() + (v + 1) * frameFloats, static_cast<float*>(a->data()));
        a->globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(samplesSqrt * samplesSqrt));
        a->globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
        a->globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
        a->globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
        a->globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
        a->globalTagList().set("WURBLPT/DEVICE_MODEL", wpt_device_name(device));
        a->globalTagList().set("WURBLPT/DEVICE_COUNT", "1");
        a->globalTagList().set("WURBLPT/DEVICE_SECONDS", seconds);
    }
}

/* mcpt() with a sample-count map (adaptive sampling, wurblpt_hip.h: wpt_render_adaptive_block), on one device.
 * samplesSqrt holds n_p for every pixel, [height][width] with row 0 at the bottom like the frame: pixel p gets n_p^2 samples
 * and is bit for bit what mcpt(sensor, ..., n_p, ...) writes; a pixel with n_p = 0 is not rendered and keeps the value the
 * sensor held.  `moments` (may be NULL) receives the moment film, width x height x 3: per channel, 1 / n_p^2 times the sum over
 * the samples of the square of what each sample added; a pixel with n_p = 0 keeps its entries where `moments` already has the
 * frame's size (otherwise it is made anew, with zeros).  A map of the wrong size is refused before any device work
 * (std::invalid_argument).  The tags are the plain render's, but WURBLPT/SAMPLES_PER_PIXEL is "adaptive" and
 * WURBLPT/SAMPLES_TOTAL is the sum of n_p^2. */
inline void mcpt(SensorRGB& sensor, const Camera& camera, const Scene& scene, const std::vector<uint16_t>& samplesSqrt,
        float t0 = 0.0f, float t1 = 0.0f, const Parameters& params = Parameters(), Array<float>* moments = nullptr)
{
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    if (samplesSqrt.size() != size_t(width) * height)
        throw std::invalid_argument("mcpt: the sample-count map must hold one count per pixel (width * height)");
    if (scene.bvhNeedsUpdate(t0, t1))
        mcptFatal("Scene::updateBVH(t0, t1) must run before mcpt()");
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    if (camera.animation) {
        cam.animation = flat.addAnimation(camera.animation.get());
        if (cam.animation < 0)
            mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
    }
    const wpt_scene_desc desc = flat.desc();
    wpt_params p = makeParams(params, sensor);
    p.t0 = t0;
    p.t1 = t1;
    uint64_t total = 0;
    for (uint16_t n : samplesSqrt)
        total += uint64_t(n) * n;

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %llu samples in all (adaptive).\n", width, height, static_cast<unsigned long long>(total));
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());
    if (moments && (moments->dimension(0) != width || moments->dimension(1) != height || moments->componentCount() != 3))
        *moments = Array<float>(width, height, 3);
    ArrayContainer* a = sensor.pixelArray();
    const auto renderStart = std::chrono::steady_clock::now();
    wpt_scene* dscene = nullptr;
    if (wpt_scene_upload(&desc, &dscene) != WPT_OK)
        mcptFatal(wpt_last_error());
    const wpt_status st = wpt_render_adaptive_block(dscene, &cam, &p, width, height, samplesSqrt.data(), 0, width * height,
            static_cast<float*>(a->data()), moments ? static_cast<float*>(moments->data()) : nullptr);
    wpt_scene_free(dscene);
    if (st != WPT_OK)
        mcptFatal(wpt_last_error());

    int device = 0;
    if (wpt_current_device(&device) != WPT_OK)
        device = 0;
    a->globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", "adaptive");
    a->globalTagList().set("WURBLPT/SAMPLES_TOTAL", std::to_string(total));
    a->globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
    a->globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
    a->globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
    a->globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
    a->globalTagList().set("WURBLPT/DEVICE_MODEL", wpt_device_name(device));
    a->globalTagList().set("WURBLPT/DEVICE_COUNT", "1");
    a->globalTagList().set("WURBLPT/DEVICE_SECONDS",
            std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count()));
}

/* A sample-count map for mcpt() with a map, from a pilot render with pilotSamplesSqrt^2 samples (>= 2, so that a variance can
 * be estimated) and its moment film: for every pixel, in float64,
 *   N0 = pilot^2;  var_c = max(m_c - f_c^2, 0) * (N0 / (N0 - 1))  (the pixel's sample variance);
 *   need = max over c of var_c / (relError^2 * max(|f_c|, floor)^2);
 *   n = clamp(ceil(sqrt(need)), minSqrt, maxSqrt),
 * so that the standard error of the mean, sqrt(var_c / n^2), is about relError times the value (or times `floor` where the value
 * is smaller).  A pixel with a non-finite input, or a non-finite `need`, gets maxSqrt.  Refused (std::invalid_argument): a pilot
 * below 2, arrays that differ in size or are not three channels, relError not > 0, floor not >= 0, minSqrt > maxSqrt or
 * maxSqrt > 65535.  wurblpt_amd.device.samples_sqrt_for_error is the same formula. */
inline std::vector<uint16_t> samplesSqrtForError(const Array<float>& frame, const Array<float>& moments, unsigned int pilotSamplesSqrt,
        double relError, unsigned int minSqrt, unsigned int maxSqrt, double floor)
{
    if (pilotSamplesSqrt < 2)
        throw std::invalid_argument("samplesSqrtForError: the pilot needs pilotSamplesSqrt >= 2");
    if (frame.dimension(0) != moments.dimension(0) || frame.dimension(1) != moments.dimension(1) || frame.componentCount() != 3
            || moments.componentCount() != 3)
        throw std::invalid_argument("samplesSqrtForError: frame and moments must be arrays of one size with three channels");
    if (!(relError > 0.0) || !(floor >= 0.0) || minSqrt > maxSqrt || maxSqrt > 65535)
        throw std::invalid_argument("samplesSqrtForError: needs relError > 0, floor >= 0 and minSqrt <= maxSqrt <= 65535");
    const double N0 = double(pilotSamplesSqrt) * double(pilotSamplesSqrt);
    const double scale = N0 / (N0 - 1.0);
    const double r2 = relError * relError;
    const size_t pixels = frame.elementCount();
    std::vector<uint16_t> map(pixels);
    for (size_t i = 0; i < pixels; i++) {
        const float* f = frame[i];
        const float* m = moments[i];
        bool finite = true;
        double need = 0.0;
        for (int c = 0; c < 3 && finite; c++) {
            const double fc = f[c], mc = m[c];
            if (!std::isfinite(fc) || !std::isfinite(mc)) {
                finite = false;
                break;
            }
            const double var = std::max(mc - fc * fc, 0.0) * scale;
            const double d = std::max(std::fabs(fc), floor);
            const double q = var / (r2 * (d * d));
            if (!std::isfinite(q))
                finite = false;
            else if (c == 0 || q > need)
                need = q;
        }
        unsigned int n = maxSqrt;
        if (finite) {
            const double s = std::ceil(std::sqrt(need));
            n = s < double(minSqrt) ? minSqrt : s > double(maxSqrt) ? maxSqrt : static_cast<unsigned int>(s);
        }
        map[i] = static_cast<uint16_t>(n);
    }
    return map;
}

/* mcpt() for a SensorRGBTransient: the frame and every bin in one pass per block (wurblpt_hip.h: wpt_render_transient_block).
 * Each worker renders the blocks it takes from the coordinator, several devices included, and writes their pixels of the frame
 * and of every bin. */
inline void mcptTransient(MPICoordinator& mpiCoordinator, SensorRGBTransient& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0, float t1, const Parameters& params)
{
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    if (camera.animation) {
        cam.animation = flat.addAnimation(camera.animation.get());
        if (cam.animation < 0)
            mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
    }
    const wpt_scene_desc desc = flat.desc();
    SensorRGB gates(1, 1, sensor.minDistToLight, sensor.maxDistToLight); /* the frame: the distance gate only */
    wpt_params p = makeParams(params, gates);
    p.t0 = t0;
    p.t1 = t1;
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    const unsigned int binCount = sensor.binCount();
    const std::vector<float>& edges = sensor.binEdges();
    ArrayContainer* pixelArray = sensor.pixelArray();

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples into the frame and %u path length bins.\n", width, height,
            samplesSqrt * samplesSqrt, binCount);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());

    mpiCoordinator.init(width, height, static_cast<float*>(pixelArray->data()), pixelArray->componentCount());
    std::vector<std::string> workerErrors(mpiCoordinator.devices().size());
    const auto renderStart = std::chrono::steady_clock::now();
    auto worker = [&](size_t w) {
        int device = mpiCoordinator.devices()[w];
        if (device >= 0 && wpt_select_device(device) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        wpt_scene* dscene = nullptr;
        if (wpt_scene_upload(&desc, &dscene) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        std::vector<float> blockBins;
        for (;;) {
            unsigned int blockStart, blockSize;
            mpiCoordinator.getBlock(&blockStart, &blockSize);
            if (blockSize == 0)
                break;
            fprintf(stderr, "%s: device %d renders block of size %u starting at %u\n", mpiCoordinator.processId(), device, blockSize, blockStart);
            blockBins.resize(size_t(binCount) * blockSize * 3);
            if (wpt_render_transient_block(dscene, &cam, &p, edges.data(), binCount, width, height, samplesSqrt, blockStart, blockSize,
                        mpiCoordinator.blockData(blockStart), blockBins.data()) != WPT_OK) {
                workerErrors[w] = wpt_last_error();
                break;
            }
            for (unsigned int k = 0; k < binCount; k++)
                std::copy(blockBins.begin() + size_t(k) * blockSize * 3, blockBins.begin() + size_t(k + 1) * blockSize * 3,
                        static_cast<float*>(sensor.bin(k).data()) + size_t(blockStart) * 3);
            mpiCoordinator.submitBlock(blockStart, blockSize);
        }
        wpt_scene_free(dscene);
    };
    if (mpiCoordinator.devices().size() == 1) {
        worker(0);
    } else {
        std::vector<std::thread> threads;
        for (size_t w = 0; w < mpiCoordinator.devices().size(); w++)
            threads.emplace_back(worker, w);
        for (auto& t : threads)
            t.join();
    }
    mpiCoordinator.finish();
    for (const std::string& e : workerErrors)
        if (!e.empty())
            mcptFatal(e);

    std::string deviceModel;
    for (int device : mpiCoordinator.devices()) {
        int current = device;
        if (current < 0 && wpt_current_device(&current) != WPT_OK)
            current = 0;
        deviceModel += (deviceModel.empty() ? "" : "; ") + std::string(wpt_device_name(current));
    }
    const std::string seconds = std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count());
    auto runTags = [&](ArrayContainer& a) {
        a.globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(samplesSqrt * samplesSqrt));
        a.globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
        a.globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
        a.globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
        a.globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
        a.globalTagList().set("WURBLPT/DEVICE_MODEL", deviceModel);
        a.globalTagList().set("WURBLPT/DEVICE_COUNT", std::to_string(mpiCoordinator.devices().size()));
        a.globalTagList().set("WURBLPT/DEVICE_SECONDS", seconds);
    };
    runTags(*pixelArray);
    char edge[32];
    for (unsigned int k = 0; k < binCount; k++) {
        runTags(sensor.bin(k));
        sensor.bin(k).globalTagList().set("WURBLPT/TRANSIENT_BIN", std::to_string(k));
        snprintf(edge, sizeof(edge), "%.9g", edges[k]);
        sensor.bin(k).globalTagList().set("WURBLPT/TRANSIENT_MIN_PATH_LEN", edge);
        snprintf(edge, sizeof(edge), "%.9g", edges[k + 1]);
        sensor.bin(k).globalTagList().set("WURBLPT/TRANSIENT_MAX_PATH_LEN", edge); /* exclusive */
    }
}

/* The table a light-groups launch takes (wurblpt_hip.h): the group of every flattened material record.  The sensor's
 * assignments name Materials; a record is found through Scene::materialIndex().  A MaterialTwoSided's assignment goes to both
 * its children first, assignments of other materials after it; what nobody assigned is in group 0. */
inline std::vector<uint8_t> lightGroupsTable(const SensorRGBLightGroups& sensor, const Scene& scene, const FlatScene& flat)
{
    std::map<int, unsigned int> groupOfSceneIndex;
    auto spread = [&](auto&& self, const Material* m, unsigned int g, int depth) -> void {
        const MaterialTwoSided* two = dynamic_cast<const MaterialTwoSided*>(m);
        if (two && depth < 4) {
            self(self, two->frontSideMaterial(), g, depth + 1);
            self(self, two->backSideMaterial(), g, depth + 1);
        }
        const int index = scene.materialIndex(m);
        if (index >= 0)
            groupOfSceneIndex[index] = g;
    };
    for (const auto& entry : sensor.assignments())
        if (dynamic_cast<const MaterialTwoSided*>(entry.first))
            spread(spread, entry.first, entry.second, 0);
    for (const auto& entry : sensor.assignments())
        if (!dynamic_cast<const MaterialTwoSided*>(entry.first))
            spread(spread, entry.first, entry.second, 0);
    std::vector<uint8_t> table(flat.materials.size(), 0);
    for (size_t i = 0; i < table.size(); i++) {
        auto it = groupOfSceneIndex.find(flat.materialSceneIndex[i]);
        if (it != groupOfSceneIndex.end())
            table[i] = uint8_t(it->second);
    }
    return table;
}

/* mcpt() for a SensorRGBLightGroups: the frame and every group's frame in one pass per block (wurblpt_hip.h:
 * wpt_render_light_groups_block), the blocks handed out by the coordinator as for the transient film. */
inline void mcptLightGroups(MPICoordinator& mpiCoordinator, SensorRGBLightGroups& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0, float t1, const Parameters& params)
{
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    if (camera.animation) {
        cam.animation = flat.addAnimation(camera.animation.get());
        if (cam.animation < 0)
            mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
    }
    const wpt_scene_desc desc = flat.desc();
    SensorRGB gates(1, 1, sensor.minDistToLight, sensor.maxDistToLight, sensor.minPathLen, sensor.maxPathLen);
    wpt_params p = makeParams(params, gates);
    p.t0 = t0;
    p.t1 = t1;
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    const unsigned int groupCount = sensor.groupCount();
    const std::vector<uint8_t> table = lightGroupsTable(sensor, scene, flat);
    ArrayContainer* pixelArray = sensor.pixelArray();

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples into the frame and %u light groups.\n", width, height,
            samplesSqrt * samplesSqrt, groupCount);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());

    mpiCoordinator.init(width, height, static_cast<float*>(pixelArray->data()), pixelArray->componentCount());
    std::vector<std::string> workerErrors(mpiCoordinator.devices().size());
    const auto renderStart = std::chrono::steady_clock::now();
    auto worker = [&](size_t w) {
        int device = mpiCoordinator.devices()[w];
        if (device >= 0 && wpt_select_device(device) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        wpt_scene* dscene = nullptr;
        if (wpt_scene_upload(&desc, &dscene) != WPT_OK) {
            workerErrors[w] = wpt_last_error();
            return;
        }
        std::vector<float> blockPlanes;
        for (;;) {
            unsigned int blockStart, blockSize;
            mpiCoordinator.getBlock(&blockStart, &blockSize);
            if (blockSize == 0)
                break;
            fprintf(stderr, "%s: device %d renders block of size %u starting at %u\n", mpiCoordinator.processId(), device, blockSize, blockStart);
            blockPlanes.resize(size_t(groupCount) * blockSize * 3);
            if (wpt_render_light_groups_block(dscene, &cam, &p, table.data(), uint32_t(table.size()), groupCount, sensor.environmentGroup(),
                        width, height, samplesSqrt, blockStart, blockSize, mpiCoordinator.blockData(blockStart), blockPlanes.data()) != WPT_OK) {
                workerErrors[w] = wpt_last_error();
                break;
            }
            for (unsigned int g = 0; g < groupCount; g++)
                std::copy(blockPlanes.begin() + size_t(g) * blockSize * 3, blockPlanes.begin() + size_t(g + 1) * blockSize * 3,
                        static_cast<float*>(sensor.group(g).data()) + size_t(blockStart) * 3);
            mpiCoordinator.submitBlock(blockStart, blockSize);
        }
        wpt_scene_free(dscene);
    };
    if (mpiCoordinator.devices().size() == 1) {
        worker(0);
    } else {
        std::vector<std::thread> threads;
        for (size_t w = 0; w < mpiCoordinator.devices().size(); w++)
            threads.emplace_back(worker, w);
        for (auto& t : threads)
            t.join();
    }
    mpiCoordinator.finish();
    for (const std::string& e : workerErrors)
        if (!e.empty())
            mcptFatal(e);

    std::string deviceModel;
    for (int device : mpiCoordinator.devices()) {
        int current = device;
        if (current < 0 && wpt_current_device(&current) != WPT_OK)
            current = 0;
        deviceModel += (deviceModel.empty() ? "" : "; ") + std::string(wpt_device_name(current));
    }
    const std::string seconds = std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count());
    auto runTags = [&](ArrayContainer& a) {
        a.globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(samplesSqrt * samplesSqrt));
        a.globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
        a.globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
        a.globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
        a.globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
        a.globalTagList().set("WURBLPT/DEVICE_MODEL", deviceModel);
        a.globalTagList().set("WURBLPT/DEVICE_COUNT", std::to_string(mpiCoordinator.devices().size()));
        a.globalTagList().set("WURBLPT/DEVICE_SECONDS", seconds);
    };
    runTags(*pixelArray);
    for (unsigned int g = 0; g < groupCount; g++) {
        runTags(sensor.group(g));
        sensor.group(g).globalTagList().set("WURBLPT/LIGHT_GROUP", std::to_string(g));
    }
}

inline void mcpt(Sensor& sensor, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0 = 0.0f,
        float t1 = 0.0f, const Parameters& params = Parameters())
{
    MPICoordinator mpiCoordinator;
    mcpt(mpiCoordinator, sensor, camera, scene, samplesSqrt, t0, t1, params);
}

/* Ground Truth generation (reference: wurblpt.hpp:453-769).  One ray through the centre of every pixel
 * on the device (wpt_ground_truth, wurblpt_hip.h); the arrays a caller did not ask for stay empty. */

class GroundTruth
{
public:
    static constexpr unsigned int WorldSpacePositions         = (1 << 0);
    static constexpr unsigned int WorldSpaceGeometryNormals   = (1 << 1);
    static constexpr unsigned int WorldSpaceGeometryTangents  = (1 << 2);
    static constexpr unsigned int WorldSpaceMaterialNormals   = (1 << 3);
    static constexpr unsigned int WorldSpaceMaterialTangents  = (1 << 4);
    static constexpr unsigned int CameraSpacePositions        = (1 << 5);
    static constexpr unsigned int CameraSpaceGeometryNormals  = (1 << 6);
    static constexpr unsigned int CameraSpaceGeometryTangents = (1 << 7);
    static constexpr unsigned int CameraSpaceMaterialNormals  = (1 << 8);
    static constexpr unsigned int CameraSpaceMaterialTangents = (1 << 9);
    static constexpr unsigned int CameraSpaceDepths           = (1 << 10);
    static constexpr unsigned int CameraSpaceDistances        = (1 << 11);
    static constexpr unsigned int TexCoords                   = (1 << 12);
    static constexpr unsigned int WorldSpaceOffsetToPrev      = (1 << 13);
    static constexpr unsigned int WorldSpaceOffsetToNext      = (1 << 14);
    static constexpr unsigned int CameraSpaceOffsetToPrev     = (1 << 15);
    static constexpr unsigned int CameraSpaceOffsetToNext     = (1 << 16);
    static constexpr unsigned int PixelSpaceOffsetToPrev      = (1 << 17);
    static constexpr unsigned int PixelSpaceOffsetToNext      = (1 << 18);
    static constexpr unsigned int Materials                   = (1 << 19);
    static constexpr unsigned int All                         = (1 << 20) - 1;

    unsigned int bits;
    Array<float> worldSpacePositions;
    Array<float> worldSpaceGeometryNormals;
    Array<float> worldSpaceGeometryTangents;
    Array<float> worldSpaceMaterialNormals;
    Array<float> worldSpaceMaterialTangents;
    Array<float> cameraSpacePositions;
    Array<float> cameraSpaceGeometryNormals;
    Array<float> cameraSpaceGeometryTangents;
    Array<float> cameraSpaceMaterialNormals;
    Array<float> cameraSpaceMaterialTangents;
    Array<float> cameraSpaceDepths;    // == -cameraSpacePosition.z
    Array<float> cameraSpaceDistances; // == length(cameraSpacePosition)
    Array<float> texCoords;
    Array<float> worldSpaceOffsetToPrev;
    Array<float> worldSpaceOffsetToNext;
    Array<float> cameraSpaceOffsetToPrev;
    Array<float> cameraSpaceOffsetToNext;
    Array<float> pixelSpaceOffsetToPrev;
    Array<float> pixelSpaceOffsetToNext;
    Array<int32_t> materials;          // Scene::materialIndex() of the hitable's material, -1 where nothing is hit

    GroundTruth() : bits(0) {}

    GroundTruth(unsigned int width, unsigned int height, unsigned int bits = All) : bits(bits)
    {
        Array<float>* f[19] = { &worldSpacePositions, &worldSpaceGeometryNormals, &worldSpaceGeometryTangents,
            &worldSpaceMaterialNormals, &worldSpaceMaterialTangents, &cameraSpacePositions, &cameraSpaceGeometryNormals,
            &cameraSpaceGeometryTangents, &cameraSpaceMaterialNormals, &cameraSpaceMaterialTangents, &cameraSpaceDepths,
            &cameraSpaceDistances, &texCoords, &worldSpaceOffsetToPrev, &worldSpaceOffsetToNext, &cameraSpaceOffsetToPrev,
            &cameraSpaceOffsetToNext, &pixelSpaceOffsetToPrev, &pixelSpaceOffsetToNext };
        for (int k = 0; k < 19; k++)
            if (bits & (1u << k))
                *f[k] = Array<float>(width, height, wpt_gt_components[k]);
        if (bits & Materials)
            materials = Array<int32_t>(width, height, 1);
    }

    /* the arrays in the order of the bits, as wpt_ground_truth takes them (NULL where not asked for) */
    void arrayPointers(void* out[WPT_GT_ARRAY_COUNT])
    {
        ArrayContainer* a[WPT_GT_ARRAY_COUNT] = { &worldSpacePositions, &worldSpaceGeometryNormals, &worldSpaceGeometryTangents,
            &worldSpaceMaterialNormals, &worldSpaceMaterialTangents, &cameraSpacePositions, &cameraSpaceGeometryNormals,
            &cameraSpaceGeometryTangents, &cameraSpaceMaterialNormals, &cameraSpaceMaterialTangents, &cameraSpaceDepths,
            &cameraSpaceDistances, &texCoords, &worldSpaceOffsetToPrev, &worldSpaceOffsetToNext, &cameraSpaceOffsetToPrev,
            &cameraSpaceOffsetToNext, &pixelSpaceOffsetToPrev, &pixelSpaceOffsetToNext, &materials };
        for (int k = 0; k < WPT_GT_ARRAY_COUNT; k++)
            out[k] = (bits & (1u << k)) ? a[k]->data() : nullptr;
    }
};

/* The picture is taken at t0; the flow arrays compare with tPrev and tNext: the camera at those times (its animation,
 * or cameraPrev / cameraNext where an application keeps separate camera objects per frame) and the places the hit
 * points of animated instances have then (wurblpt.hpp:626-761). */
inline GroundTruth getGroundTruth(const Sensor& sensor, const Camera& camera, const Camera* cameraPrev, const Camera* cameraNext,
        const Scene& scene, float t0, float tPrev, float tNext, unsigned int groundTruthBits = GroundTruth::All,
        const Parameters& params = Parameters())
{
    if (scene.bvhNeedsUpdate(t0, t0))
        mcptFatal("Scene::updateBVH() must run before getGroundTruth()");
    wpt_camera cam, camPrev, camNext;
    if (!camera.describe(cam, t0) || !(cameraPrev ? cameraPrev->describe(camPrev, tPrev) : camera.describe(camPrev, tPrev))
            || !(cameraNext ? cameraNext->describe(camNext, tNext) : camera.describe(camNext, tNext)))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    const wpt_scene_desc desc = flat.desc();
    wpt_params p;
    p.max_path_components = params.maxPathComponents;
    p.rr_threshold = params.rrThreshold;
    p.randomize_ray_over_pixel = 0;
    p.min_hit_distance = params.minHitDistance;
    p.min_dist_to_light = 0.0f;
    p.max_dist_to_light = std::numeric_limits<float>::max();
    p.min_path_len = 0.0f;
    p.max_path_len = std::numeric_limits<float>::max();
    p.t0 = t0;
    p.t1 = t0;
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    GroundTruth gt(width, height, groundTruthBits);
    fprintf(stderr, "Getting ground truth for %ux%u pixels at %.3fs... ", width, height, t0);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());
    wpt_scene* dscene = nullptr;
    if (wpt_scene_upload(&desc, &dscene) != WPT_OK)
        mcptFatal(wpt_last_error());
    void* arrays[WPT_GT_ARRAY_COUNT];
    gt.arrayPointers(arrays);
    const float times[3] = { t0, tPrev, tNext };
    const wpt_status st = wpt_ground_truth(dscene, &cam, &camPrev, &camNext, times, &p, width, height, arrays);
    wpt_scene_free(dscene);
    if (st != WPT_OK)
        mcptFatal(wpt_last_error());
    /* the kernel reports positions in the flattened material list; the reference reports Scene::materialIndex() */
    if (groundTruthBits & GroundTruth::Materials) {
        for (size_t i = 0; i < gt.materials.elementCount(); i++) {
            int32_t& m = gt.materials[i][0];
            m = (m >= 0 && size_t(m) < flat.materialSceneIndex.size()) ? flat.materialSceneIndex[m] : -1;
        }
    }
    fprintf(stderr, "done\n");
    return gt;
}

inline GroundTruth getGroundTruth(const Sensor& sensor, const Camera& camera, const Scene& scene, float t0, float tPrev,
        float tNext, unsigned int groundTruthBits = GroundTruth::All, const Parameters& params = Parameters())
{
    return getGroundTruth(sensor, camera, nullptr, nullptr, scene, t0, tPrev, tNext, groundTruthBits, params);
}

inline GroundTruth getGroundTruth(const Sensor& sensor, const Camera& camera, const Scene& scene, float t0 = 0.0f,
        unsigned int groundTruthBits = GroundTruth::All, const Parameters& params = Parameters())
{
    return getGroundTruth(sensor, camera, scene, t0, t0, t0, groundTruthBits, params);
}

/* What the surface behind every pixel's centre multiplies the light with (albedo) and what it emits itself (emission), with the
 * three arrays of a GroundTruth a denoiser reads, all from one walk per pixel on the device (wpt_first_hit_colours,
 * wurblpt_hip.h, which has the rule per material).  denoise(..., albedo, emission, ...) takes them (postproc.hpp). */
class FirstHitColours
{
public:
    Array<float> albedo;                     // 3 components
    Array<float> emission;                   // 3
    Array<float> cameraSpacePositions;       // as GroundTruth's
    Array<float> cameraSpaceMaterialNormals;
    Array<int32_t> materials;                // Scene::materialIndex() of the hitable's material, -1 where nothing is hit
};

inline FirstHitColours getFirstHitColours(unsigned int width, unsigned int height, const Camera& camera, const Scene& scene, float t0 = 0.0f,
        const Parameters& params = Parameters())
{
    if (scene.bvhNeedsUpdate(t0, t0))
        mcptFatal("Scene::updateBVH() must run before getFirstHitColours()");
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    const wpt_scene_desc desc = flat.desc();
    wpt_params p;
    p.max_path_components = params.maxPathComponents;
    p.rr_threshold = params.rrThreshold;
    p.randomize_ray_over_pixel = 0;
    p.min_hit_distance = params.minHitDistance;
    p.min_dist_to_light = 0.0f;
    p.max_dist_to_light = std::numeric_limits<float>::max();
    p.min_path_len = 0.0f;
    p.max_path_len = std::numeric_limits<float>::max();
    p.t0 = t0;
    p.t1 = t0;
    FirstHitColours fh;
    fh.albedo = Array<float>(width, height, 3);
    fh.emission = Array<float>(width, height, 3);
    fh.cameraSpacePositions = Array<float>(width, height, 3);
    fh.cameraSpaceMaterialNormals = Array<float>(width, height, 3);
    fh.materials = Array<int32_t>(width, height, 1);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());
    wpt_scene* dscene = nullptr;
    if (wpt_scene_upload(&desc, &dscene) != WPT_OK)
        mcptFatal(wpt_last_error());
    void* guide[3] = { fh.cameraSpacePositions.data(), fh.cameraSpaceMaterialNormals.data(), fh.materials.data() };
    const wpt_status st = wpt_first_hit_colours(dscene, &cam, &p, width, height, static_cast<float*>(fh.albedo.data()),
            static_cast<float*>(fh.emission.data()), guide);
    wpt_scene_free(dscene);
    if (st != WPT_OK)
        mcptFatal(wpt_last_error());
    /* the kernel reports positions in the flattened material list; the reference reports Scene::materialIndex() */
    for (size_t i = 0; i < fh.materials.elementCount(); i++) {
        int32_t& m = fh.materials[i][0];
        m = (m >= 0 && size_t(m) < flat.materialSceneIndex.size()) ? flat.materialSceneIndex[m] : -1;
    }
    return fh;
}

inline FirstHitColours getFirstHitColours(const Sensor& sensor, const Camera& camera, const Scene& scene, float t0 = 0.0f,
        const Parameters& params = Parameters())
{
    return getFirstHitColours(sensor.width(), sensor.height(), camera, scene, t0, params);
}

}
