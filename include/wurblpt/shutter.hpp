/*
 * shutter.hpp -- the rolling shutter: a frame whose rows are exposed one after the other, as a CMOS sensor reads them out.
 *
 * Not included by wurblpt.hpp: an application includes it next to that header.  mcpt() exposes every row of the frame over
 * [t0, t1]; mcptRollingShutter() exposes the row at place k of the readout (k = 0: the row read first) over
 * [t0 + k * rowTime, t1 + k * rowTime], each product and each sum rounded to float once (wurblpt_hip.h has the rule as the
 * kernels apply it, wpt_shutter_row_interval evaluates it).  A row of the rolling frame is bit for bit that row of the mcpt()
 * frame with the row's interval.  With t0 == t1 the rows are instants: the classic skew and wobble without motion blur, the
 * camera taken where its animation has it at each row's time.
 *
 * The scene must be bounded for the whole readout, [t0, shutter.end(t0, t1, height)], not for [t0, t1]: moving triangles
 * whose boxes cover less are missed without a word, so mcptRollingShutter() checks it first and is fatal otherwise.
 * One frame from a SensorRGB; the other sensors, batches of views and getGroundTruth() take no shutter.
 */
#pragma once

#include <string>
#include <thread>
#include <vector>

#include "wurblpt.hpp"

namespace WurblPT {

struct RollingShutter {
    float rowTime = 0.0f; /* between two rows of the readout; 0: a global shutter */
    bool fromTop = true;  /* the top row of the picture is read first */

    wpt_shutter describe() const
    {
        wpt_shutter s = {};
        s.row_time = rowTime;
        s.from_top = fromTop ? 1u : 0u;
        return s;
    }

    /* when the row read last closes: the readout of a frame of `height` rows exposed over [t0, t1] spans [t0, end] */
    float end(float t0, float t1, unsigned int height) const
    {
        const wpt_shutter s = describe();
        float first = 0.0f, last = 0.0f;
        if (wpt_shutter_span(&s, t0, t1, height, &first, &last) != WPT_OK)
            mcptFatal(wpt_last_error());
        return last;
    }
};

inline void mcptRollingShutter(MPICoordinator& mpiCoordinator, SensorRGB& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0, float t1, const RollingShutter& shutter, const Parameters& params = Parameters())
{
    const unsigned int width = sensor.width();
    const unsigned int height = sensor.height();
    const float end = shutter.end(t0, t1, height); /* (fatal for a shutter the library refuses) */
    if (scene.bvhNeedsUpdate(t0, end))
        mcptFatal("Scene::updateBVH(t0, shutter.end(...)) must run before mcptRollingShutter()");
    const wpt_shutter rows = shutter.describe();
    wpt_camera cam;
    if (!camera.describe(cam, t0))
        mcptFatal("this camera cannot be described to the device path");
    FlatScene flat;
    std::string error;
    if (!scene.flatten(flat, &error))
        mcptFatal(error);
    if (camera.animation) {
        /* the camera's key frames join the scene's pool; every row takes them at its own time */
        cam.animation = flat.addAnimation(camera.animation.get());
        if (cam.animation < 0)
            mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
    }
    const wpt_scene_desc desc = flat.desc();
    wpt_params p = makeParams(params, sensor);
    p.t0 = t0;
    p.t1 = t1;
    ArrayContainer* pixelArray = sensor.pixelArray();

    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples, rows read from the %s every %g s.\n", width, height, samplesSqrt * samplesSqrt,
            shutter.fromTop ? "top" : "bottom", shutter.rowTime);
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
            /* several devices: each takes its bands of 16 rows in one launch, as in mcpt(); a band's rows keep the places they
             * have in the frame's readout */
            const unsigned int count = mpiCoordinator.devices().size();
            fprintf(stderr, "%s: device %d renders bands %zu, %zu, ... of 16 rows\n", mpiCoordinator.processId(), device, w, w + count);
            if (wpt_render_shutter_bands(dscene, &cam, &p, &rows, width, height, samplesSqrt, 16, w, count, mpiCoordinator.blockData(0)) != WPT_OK)
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
            /* (a block names its pixels by their index in the frame: its rows are the frame's) */
            if (wpt_render_shutter_block(dscene, &cam, &p, &rows, width, height, samplesSqrt, blockStart, blockSize,
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

    std::string deviceModel;
    for (int device : mpiCoordinator.devices()) {
        int current = device;
        if (current < 0 && wpt_current_device(&current) != WPT_OK)
            current = 0;
        deviceModel += (deviceModel.empty() ? "" : "; ") + std::string(wpt_device_name(current));
    }
    auto& tags =pixelArray->globalTagList();
    tags.set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(samplesSqrt * samplesSqrt));
    tags.set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(params.maxPathComponents));
    tags.set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(params.rrThreshold));
    tags.set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
    tags.set("WURBLPT/COMPILER", wpt_build_info());
    tags.set("WURBLPT/DEVICE_MODEL", deviceModel);
    tags.set("WURBLPT/DEVICE_COUNT", std::to_string(mpiCoordinator.devices().size()));
    tags.set("WURBLPT/DEVICE_SECONDS", std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count()));
    char number[32];
    snprintf(number, sizeof(number), "%.9g", shutter.rowTime);
    tags.set("WURBLPT/SHUTTER_ROW_TIME", number);
    tags.set("WURBLPT/SHUTTER_FROM_TOP", shutter.fromTop ? "1" : "0");
    snprintf(number, sizeof(number), "%.9g", end);
    tags.set("WURBLPT/SHUTTER_END", number);
}

inline void mcptRollingShutter(SensorRGB& sensor, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0, float t1,
        const RollingShutter& shutter, const Parameters& params = Parameters())
{
    MPICoordinator mpiCoordinator;
    mcptRollingShutter(mpiCoordinator, sensor, camera, scene, samplesSqrt, t0, t1, shutter, params);
}

}
