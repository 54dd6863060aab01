/*
 * progressive.hpp -- a frame in resumable stages: ProgressiveRender and the mcpt() that reports every stage
 * (wurblpt_hip.h: wpt_progress_*).
 *
 * Not included by wurblpt.hpp: an application includes it next to that header.  A session renders rows of strata of every
 * pixel, stage by stage; a pixel's samples stay one sequence from one generator, so the finished frame is bit for bit the
 * frame of mcpt(), however the rows are cut into stages and whether or not the session was saved to a file and resumed in
 * another process in between.  preview() is the mean over the strata rendered so far, which after r of n rows are the lower
 * r / n of every pixel's strata: a picture to look at, not an estimate to publish.  A session holds 40 bytes of device
 * memory per pixel and the uploaded scene for its lifetime.  One device; there is no CPU fallback.
 */
#pragma once

#include <cstdint>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "wurblpt.hpp"

namespace WurblPT {

/* The fingerprint of a flattened scene that a saved session carries: FNV-1a (64 bit) over the description's arrays in this
 * order -- nodes, tri_geom, tri_attr, instances, materials, textures, texels, hotspots, spheres, rgl_brdfs, rgl_data,
 * animations, keyframes -- each as the 8 bytes of its length in bytes (little endian) followed by its bytes, then the
 * environment map's type, compat, tex, N and cube_tex (40 bytes).  wurblpt_amd.host.scene_tag is the same function. */
inline uint64_t sceneTag(const wpt_scene_desc& d)
{
    uint64_t h = 0xcbf29ce484222325ull;
    auto bytes = [&h](const void* p, uint64_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (uint64_t i = 0; i < n; i++)
            h = (h ^ b[i]) * 0x100000001b3ull;
    };
    auto array = [&bytes](const void* p, uint64_t n) {
        unsigned char len[8];
        for (int i = 0; i < 8; i++)
            len[i] = static_cast<unsigned char>(n >> (8 * i));
        bytes(len, 8);
        bytes(p, n);
    };
    array(d.nodes, uint64_t(d.node_count) * sizeof(wpt_bvh_node));
    array(d.tri_geom, uint64_t(d.tri_count) * sizeof(wpt_tri_geom));
    array(d.tri_attr, uint64_t(d.tri_count) * sizeof(wpt_tri_attr));
    array(d.instances, uint64_t(d.instance_count) * sizeof(wpt_instance));
    array(d.materials, uint64_t(d.material_count) * sizeof(wpt_material));
    array(d.textures, uint64_t(d.texture_count) * sizeof(wpt_texture));
    array(d.texels, d.texel_bytes);
    array(d.hotspots, uint64_t(d.hotspot_count) * sizeof(wpt_hotspot));
    array(d.spheres, uint64_t(d.sphere_count) * sizeof(wpt_sphere));
    array(d.rgl_brdfs, uint64_t(d.rgl_count) * sizeof(wpt_rgl_brdf));
    array(d.rgl_data, d.rgl_data_count * sizeof(float));
    array(d.animations, uint64_t(d.animation_count) * sizeof(wpt_animation));
    array(d.keyframes, uint64_t(d.keyframe_count) * sizeof(wpt_keyframe));
    bytes(&d.envmap.type, 4);
    bytes(&d.envmap.compat, 4);
    bytes(&d.envmap.tex, 4);
    bytes(&d.envmap.N, 4);
    bytes(d.envmap.cube_tex, sizeof(d.envmap.cube_tex));
    return h;
}

class ProgressiveRender
{
private:
    SensorRGB& _sensor;
    Parameters _params;
    unsigned int _samplesSqrt;
    wpt_camera _cam;
    wpt_params _p;
    uint64_t _tag;
    wpt_scene* _scene;
    wpt_progress* _progress;

    /* flattens and uploads the scene; everything a session is begun or restored with */
    void prepare(const Camera& camera, const Scene& scene, float t0, float t1)
    {
        if (scene.bvhNeedsUpdate(t0, t1))
            mcptFatal("Scene::updateBVH(t0, t1) must run before a progressive render");
        if (!camera.describe(_cam, t0))
            mcptFatal("this camera cannot be described to the device path");
        FlatScene flat;
        std::string error;
        if (!scene.flatten(flat, &error))
            mcptFatal(error);
        if (camera.animation) {
            _cam.animation = flat.addAnimation(camera.animation.get());
            if (_cam.animation < 0)
                mcptFatal("only key frame animations (AnimationKeyframes) can go to the device");
        }
        const wpt_scene_desc desc = flat.desc();
        _tag = sceneTag(desc);
        _p = makeParams(_params, _sensor);
        _p.t0 = t0;
        _p.t1 = t1;
        if (wpt_device_count() <= 0)
            mcptFatal(std::string("no HIP device: ") + wpt_last_error());
        if (wpt_scene_upload(&desc, &_scene) != WPT_OK)
            mcptFatal(wpt_last_error());
    }

    ProgressiveRender(SensorRGB& sensor, unsigned int samplesSqrt, const Parameters& params) :
        _sensor(sensor), _params(params), _samplesSqrt(samplesSqrt), _scene(nullptr), _progress(nullptr)
    {
    }

    void setTags()
    {
        ArrayContainer* a = _sensor.pixelArray();
        int device = 0;
        if (wpt_current_device(&device) != WPT_OK)
            device = 0;
        a->globalTagList().set("WURBLPT/SAMPLES_PER_PIXEL", std::to_string(_samplesSqrt * _samplesSqrt));
        a->globalTagList().set("WURBLPT/MAX_PATH_COMPONENTS", std::to_string(_params.maxPathComponents));
        a->globalTagList().set("WURBLPT/RUSSIAN_ROULETTE_THRESHOLD", std::to_string(_params.rrThreshold));
        a->globalTagList().set("WURBLPT/DEVICE_KERNEL", wpt_kernel_name());
        a->globalTagList().set("WURBLPT/COMPILER", wpt_build_info());
        a->globalTagList().set("WURBLPT/DEVICE_MODEL", wpt_device_name(device));
        a->globalTagList().set("WURBLPT/DEVICE_COUNT", "1");
    }

public:
    /* Begins a session for the whole frame of `sensor`, which must outlive it: the stage that finishes writes the frame into
     * it, with the tags of mcpt() except the seconds. */
    ProgressiveRender(SensorRGB& sensor, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0 = 0.0f, float t1 = 0.0f,
            const Parameters& params = Parameters()) :
        ProgressiveRender(sensor, samplesSqrt, params)
    {
        prepare(camera, scene, t0, t1);
        if (wpt_progress_begin(_scene, &_cam, &_p, sensor.width(), sensor.height(), samplesSqrt, 0, sensor.width() * sensor.height(), _tag,
                    &_progress) != WPT_OK) {
            const std::string error = wpt_last_error();
            wpt_scene_free(_scene);
            mcptFatal(error);
        }
    }
    ProgressiveRender(const ProgressiveRender&) = delete;
    ProgressiveRender& operator=(const ProgressiveRender&) = delete;
    ProgressiveRender(ProgressiveRender&& other) :
        _sensor(other._sensor), _params(other._params), _samplesSqrt(other._samplesSqrt), _cam(other._cam), _p(other._p), _tag(other._tag),
        _scene(other._scene), _progress(other._progress)
    {
        other._scene = nullptr;
        other._progress = nullptr;
    }
    ~ProgressiveRender()
    {
        wpt_progress_end(_progress);
        if (_scene)
            wpt_scene_free(_scene);
    }

    unsigned int rowsDone() const { return wpt_progress_rows_done(_progress); }
    unsigned int rowsTotal() const { return wpt_progress_rows_total(_progress); }
    bool finished() const { return rowsDone() == rowsTotal(); }

    /* Renders up to `rows` further rows of strata of every pixel and waits for them; returns rowsDone(). */
    unsigned int advance(unsigned int rows)
    {
        if (wpt_progress_advance(_progress, rows, static_cast<float*>(_sensor.pixelArray()->data())) != WPT_OK)
            throw std::invalid_argument(std::string("ProgressiveRender::advance: ") + wpt_last_error());
        if (finished())
            setTags();
        return rowsDone();
    }

    /* The mean over the strata rendered so far; of a finished session, its frame. */
    Array<float> preview() const
    {
        Array<float> image(_sensor.width(), _sensor.height(), 3);
        if (wpt_progress_preview(_progress, static_cast<float*>(image.data())) != WPT_OK)
            mcptFatal(wpt_last_error());
        return image;
    }

    /* Writes the session's state to a file (wurblpt_hip.h has the layout); false and a message if that fails. */
    bool save(const std::string& filename, std::string* error = nullptr) const
    {
        uint64_t bytes = 0;
        if (wpt_progress_state_bytes(_progress, &bytes) != WPT_OK)
            mcptFatal(wpt_last_error());
        std::vector<unsigned char> state(bytes);
        if (wpt_progress_save(_progress, state.data(), bytes) != WPT_OK)
            mcptFatal(wpt_last_error());
        FILE* f = fopen(filename.c_str(), "wb");
        bool ok = f && fwrite(state.data(), 1, state.size(), f) == state.size();
        if (f && fclose(f) != 0)
            ok = false;
        if (!ok && error)
            *error = filename + ": cannot write file";
        return ok;
    }

    /* The session that save() wrote, for the same sensor size, camera, scene, exposure interval and parameters: the library
     * compares them with the state and refuses one that was saved with others (std::invalid_argument names what differs, or what
     * is wrong with the file).  samplesSqrt is the state's. */
    static ProgressiveRender resume(const std::string& filename, SensorRGB& sensor, const Camera& camera, const Scene& scene, float t0 = 0.0f,
            float t1 = 0.0f, const Parameters& params = Parameters())
    {
        std::vector<unsigned char> state;
        if (!imagedetail::readFile(filename, state))
            throw std::invalid_argument("ProgressiveRender::resume: cannot read " + filename);
        wpt_progress_info info;
        if (wpt_progress_state_info(state.data(), state.size(), &info) != WPT_OK)
            throw std::invalid_argument("ProgressiveRender::resume: " + filename + ": " + wpt_last_error());
        if (info.width != sensor.width() || info.height != sensor.height() || info.block_start != 0 || info.block_size != info.width * info.height)
            throw std::invalid_argument("ProgressiveRender::resume: " + filename + ": the state was saved for a different frame size or block");
        ProgressiveRender r(sensor, info.samples_sqrt, params);
        r.prepare(camera, scene, t0, t1);
        if (wpt_progress_restore(r._scene, state.data(), state.size(), &r._cam, &r._p, r._tag, &r._progress) != WPT_OK)
            throw std::invalid_argument("ProgressiveRender::resume: " + filename + ": " + wpt_last_error());
        return r;
    }
};

/* mcpt() in stages of rowsPerStage rows of strata: onStage(rows done, preview) is called after every stage, the last
 * included, and returning false stops the render there (the sensor then holds what it held).  The finished frame goes into the
 * sensor as in mcpt(), with the same tags.  Returns true if the frame was finished. */
inline bool mcpt(SensorRGB& sensor, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0, float t1,
        const Parameters& params, const std::function<bool(unsigned int, const Array<float>&)>& onStage, unsigned int rowsPerStage = 1)
{
    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples in stages of %u rows of strata.\n", sensor.width(), sensor.height(),
            samplesSqrt * samplesSqrt, rowsPerStage);
    const auto renderStart = std::chrono::steady_clock::now();
    ProgressiveRender render(sensor, camera, scene, samplesSqrt, t0, t1, params);
    while (!render.finished()) {
        render.advance(rowsPerStage ? rowsPerStage : 1u);
        if (onStage && !onStage(render.rowsDone(), render.preview()) && !render.finished())
            return false;
    }
    sensor.pixelArray()->globalTagList().set("WURBLPT/DEVICE_SECONDS",
            std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count()));
    return true;
}

}
