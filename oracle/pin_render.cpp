/*
 * pin_render.cpp -- TEST INFRASTRUCTURE: renders the cases of pin_scenes.hpp through THIS
 * repository's headers (include/), for the tests that hold the result against the reference's
 * frames in tests/golden/frames/.  Compiled by the tests, in one of two forms:
 *
 *   default        pin_render <liboracle*.so> <tests/golden> <output directory> [one case]
 *                  Scene::flatten / Camera::describe / makeParams, then wpt_oracle_render of the
 *                  restatement library named on the command line (loaded at run time, so that
 *                  one program serves both math back ends).  No device is needed.  The
 *                  time-of-flight case is left out: the restatement has no such sensor.
 *                  Without [one case] it also answers the vectors of the reference's own classes
 *                  (tests/golden/frames/vectors_*.npy: rows of a probe's input record followed by
 *                  the reference's answer): it builds the same scene, flattens it, gives the input
 *                  records to the restatement's probe (wpt_oracle_bvh_hits, _hotspot_probe,
 *                  _material_probe, _envmap_probe) and writes the rows again with the restatement's
 *                  answer under the same file name, for the test to compare.
 *   -DPIN_DEVICE   pin_render <tests/golden> <output directory> [one case]
 *                  the product's mcpt(), linked to libwurblpt_hip.so, time of flight included
 *                  (all phase images in one launch).  Without [one case] it also answers the hit vectors
 *                  (tests/golden/frames/vectors_hits_*.npy) on the device: the scenes it builds for them are
 *                  flattened, uploaded and walked by the library's test hook wpt_selftest_hits_host (the ground
 *                  truth kernel's walk and finishHit); the rows go to <output directory>/vectors/.
 */
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <errno.h>
#include <sys/stat.h>

#include <wurblpt/wurblpt.hpp>
#include <wurblpt/tof.hpp> /* LightTof, SensorTofAmcw: the reference's umbrella header has them, this set keeps them here */

template<typename T> TGD::Array<T> pinArray(size_t width, size_t height, size_t components)
{
    return TGD::Array<T>(width, height, components);
}

#include "pin_scenes.hpp"
#include "pin_io.hpp"

using namespace WurblPT;

#ifndef PIN_DEVICE

typedef int (*RenderFn)(const wpt_scene_desc*, const wpt_camera*, const wpt_params*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
        float*, wpt_counters*, int);
typedef int (*TablesFn)(const wpt_scene_desc*, int, float*, int32_t*, float*);
typedef void (*HitsFn)(const wpt_scene_desc*, int, const float*, float*, wpt_counters*);
typedef void (*ProbeFn)(const wpt_scene_desc*, int, const float*, float*);
typedef void (*MaterialFn)(const wpt_scene_desc*, uint32_t, int, const float*, float*);

/* the restatement takes an environment map's importance tables from its caller */
struct EnvTables
{
    std::vector<float> M, Mcs;
    std::vector<int32_t> Ms;
    bool attach(wpt_scene_desc& desc, TablesFn tables)
    {
        if (desc.envmap.type == WPT_ENV_NONE || desc.envmap.N <= 0)
            return true;
        const size_t bins = size_t(desc.envmap.N) * desc.envmap.N;
        M.resize(bins);
        Ms.resize(bins);
        Mcs.resize(bins);
        if (tables(&desc, desc.envmap.N, M.data(), Ms.data(), Mcs.data()) != 0)
            return false;
        desc.envmap.M = M.data();
        desc.envmap.Ms = Ms.data();
        desc.envmap.Mcs = Mcs.data();
        return true;
    }
};

static bool answerVectors(void* lib, TablesFn tables, const std::string& goldenDir, const std::string& outDir);

int main(int argc, char* argv[])
{
    if (argc != 4 && argc != 5) {
        fprintf(stderr, "usage: %s <liboracle.so> <tests/golden> <output directory> [one case]\n", argv[0]);
        return 2;
    }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) {
        fprintf(stderr, "%s\n", dlerror());
        return 1;
    }
    RenderFn render = reinterpret_cast<RenderFn>(dlsym(lib, "wpt_oracle_render"));
    TablesFn tables = reinterpret_cast<TablesFn>(dlsym(lib, "wpt_oracle_envmap_tables"));
    if (!render || !tables)
        return 1;
    const std::string goldenDir = argv[2], outDir = argv[3];
    for (const PinScenes::Case& c : PinScenes::cases()) {
        if (c.tof || (argc == 5 && std::string(argv[4]) != c.name))
            continue;
        PinScenes::Setup s;
        PinScenes::setUp(c, s, goldenDir);
        wpt_camera cam;
        FlatScene flat;
        std::string error;
        if (!s.camera->describe(cam, c.t0) || !s.scene.flatten(flat, &error)) {
            fprintf(stderr, "%s: cannot be flattened: %s\n", c.name, error.c_str());
            return 1;
        }
        if (s.camera->animation)
            cam.animation = flat.addAnimation(s.camera->animation.get());
        wpt_scene_desc desc = flat.desc();
        EnvTables envTables;
        if (!envTables.attach(desc, tables))
            return 1;
        const SensorRGB sensor(c.width, c.height, s.minDistToLight, s.maxDistToLight, s.minPathLen, s.maxPathLen);
        wpt_params p = makeParams(s.params, sensor);
        p.t0 = c.t0;
        p.t1 = c.t1;
        std::vector<float> frame(size_t(c.width) * c.height * 3);
        const int rc = render(&desc, &cam, &p, c.width, c.height, c.samplesSqrt, 0, c.width * c.height, frame.data(), nullptr, 0);
        if (rc != 0) {
            fprintf(stderr, "%s: wpt_oracle_render returned %d\n", c.name, rc);
            return 1;
        }
        if (!PinIO::writeNpy(outDir + "/" + c.name + ".npy", { c.height, c.width, 3 }, frame.data()))
            return 1;
    }
    return (argc == 5 || answerVectors(lib, tables, goldenDir, outDir)) ? 0 : 1;
}

static bool answerVectors(void* lib, TablesFn tables, const std::string& goldenDir, const std::string& outDir)
{
    HitsFn hits = reinterpret_cast<HitsFn>(dlsym(lib, "wpt_oracle_bvh_hits"));
    ProbeFn hotSpots = reinterpret_cast<ProbeFn>(dlsym(lib, "wpt_oracle_hotspot_probe"));
    ProbeFn envmap = reinterpret_cast<ProbeFn>(dlsym(lib, "wpt_oracle_envmap_probe"));
    MaterialFn material = reinterpret_cast<MaterialFn>(dlsym(lib, "wpt_oracle_material_probe"));
    if (!hits || !hotSpots || !envmap || !material)
        return false;
    std::string error;

    /* materials: rows of 1 + 18 + 22, the first column is Scene::materialIndex() */
    {
        PinScenes::Setup s;
        s.width = 32;
        s.height = 24;
        s.goldenDir = goldenDir;
        std::vector<const Material*> list;
        PinScenes::materialsForProbe(s, list);
        s.scene.updateBVH();
        FlatScene flat;
        if (!s.scene.flatten(flat, &error)) {
            fprintf(stderr, "materials: %s\n", error.c_str());
            return false;
        }
        const wpt_scene_desc desc = flat.desc();
        std::vector<float> rows;
        if (!PinIO::readRows(goldenDir + "/frames/vectors_materials.npy", 41, rows))
            return false;
        for (size_t r = 0; r < rows.size() / 41; r++) {
            float* row = rows.data() + 41 * r;
            int flatIndex = -1;
            for (size_t k = 0; k < flat.materialSceneIndex.size(); k++)
                if (flat.materialSceneIndex[k] == int(row[0]))
                    flatIndex = int(k);
            if (flatIndex < 0) {
                fprintf(stderr, "materials: the flattened scene lacks material %d\n", int(row[0]));
                return false;
            }
            material(&desc, uint32_t(flatIndex), 1, row + 1, row + 19);
        }
        if (!PinIO::writeNpy(outDir + "/vectors_materials.npy", { rows.size() / 41, 41 }, rows.data()))
            return false;
    }

    for (const PinScenes::Probe& probe : PinScenes::probes()) {
        const PinScenes::Case& c = *PinScenes::findCase(probe.caseName);
        const std::string kind = probe.kind, name = "vectors_" + kind + "_" + c.name + ".npy";
        PinScenes::Setup s;
        PinScenes::setUp(c, s, goldenDir);
        FlatScene flat;
        if (!s.scene.flatten(flat, &error)) {
            fprintf(stderr, "%s: %s\n", c.name, error.c_str());
            return false;
        }
        wpt_scene_desc desc = flat.desc();
        EnvTables envTables;
        if (!envTables.attach(desc, tables))
            return false;
        const size_t in = kind == "hits" ? 8 : kind == "hotspots" ? 7 : 4, out = kind == "hits" ? 15 : kind == "hotspots" ? 7 : 10;
        std::vector<float> rows;
        if (!PinIO::readRows(goldenDir + "/frames/" + name, in + out, rows))
            return false;
        for (size_t r = 0; r < rows.size() / (in + out); r++) {
            float* row = rows.data() + (in + out) * r;
            if (kind == "hits") {
                hits(&desc, 1, row, row + in, nullptr);
                row[in + 1] = 0.0f; /* the index of the triangle: the reference has none to compare with */
            } else if (kind == "hotspots") {
                hotSpots(&desc, 1, row, row + in);
            } else {
                envmap(&desc, 1, row, row + in);
            }
        }
        if (!PinIO::writeNpy(outDir + "/" + name, { rows.size() / (in + out), in + out }, rows.data()))
            return false;
    }
    return true;
}

#else

static bool renderCase(const PinScenes::Case& c, const std::string& goldenDir, const std::string& fileName)
{
    PinScenes::Setup s;
    PinScenes::setUp(c, s, goldenDir);
    std::vector<float> data;
    std::vector<size_t> shape;
    if (c.tof) {
        SensorTofAmcw sensor(c.width, c.height);
        std::vector<Array<float>> energies;
        mcpt(energies, sensor, *s.camera, s.scene, c.samplesSqrt, c.t0, c.t1, s.params);
        for (const Array<float>& e : energies) {
            const float* f = static_cast<const float*>(e.data());
            data.insert(data.end(), f, f + size_t(c.width) * c.height * 3);
        }
        shape = { energies.size(), c.height, c.width, 3 };
    } else {
        SensorRGB sensor(c.width, c.height, s.minDistToLight, s.maxDistToLight, s.minPathLen, s.maxPathLen);
        mcpt(sensor, *s.camera, s.scene, c.samplesSqrt, c.t0, c.t1, s.params);
        const float* f = static_cast<const float*>(sensor.result().data());
        data.assign(f, f + size_t(c.width) * c.height * 3);
        shape = { c.height, c.width, 3 };
    }
    return PinIO::writeNpy(fileName, shape, data.data());
}

/* test hook of libwurblpt_hip.so, not part of its public header (wpt_capi_selftest.hip) */
extern "C" wpt_status wpt_selftest_hits_host(wpt_scene* scene, int n, const float* rays8_host, float* out15_host);

static bool answerHitVectors(const std::string& goldenDir, const std::string& outDir)
{
    if (mkdir(outDir.c_str(), 0777) != 0 && errno != EEXIST)
        return false;
    size_t answered = 0;
    for (const PinScenes::Probe& probe : PinScenes::probes()) {
        if (std::string(probe.kind) != "hits")
            continue;
        const PinScenes::Case& c = *PinScenes::findCase(probe.caseName);
        const std::string name = std::string("vectors_hits_") + c.name + ".npy";
        PinScenes::Setup s;
        PinScenes::setUp(c, s, goldenDir);
        FlatScene flat;
        std::string error;
        if (!s.scene.flatten(flat, &error)) {
            fprintf(stderr, "%s: %s\n", c.name, error.c_str());
            return false;
        }
        const wpt_scene_desc desc = flat.desc();
        std::vector<float> rows;
        if (!PinIO::readRows(goldenDir + "/frames/" + name, 8 + 15, rows))
            return false;
        const size_t n = rows.size() / 23;
        std::vector<float> rays(8 * n), out(15 * n);
        for (size_t r = 0; r < n; r++)
            memcpy(rays.data() + 8 * r, rows.data() + 23 * r, 8 * sizeof(float));
        wpt_scene* dscene = nullptr;
        if (wpt_scene_upload(&desc, &dscene) != WPT_OK) {
            fprintf(stderr, "%s: %s\n", c.name, wpt_last_error());
            return false;
        }
        const wpt_status st = wpt_selftest_hits_host(dscene, int(n), rays.data(), out.data());
        if (st != WPT_OK)
            fprintf(stderr, "%s: %s\n", c.name, wpt_last_error());
        wpt_scene_free(dscene);
        if (st != WPT_OK)
            return false;
        for (size_t r = 0; r < n; r++) {
            memcpy(rows.data() + 23 * r + 8, out.data() + 15 * r, 15 * sizeof(float));
            rows[23 * r + 9] = 0.0f; /* the index of the triangle: the reference has none to compare with */
        }
        if (!PinIO::writeNpy(outDir + "/" + name, { n, 23 }, rows.data()))
            return false;
        answered++;
    }
    return answered > 0;
}

int main(int argc, char* argv[])
{
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s <tests/golden> <output directory> [one case]\n", argv[0]);
        return 2;
    }
    const std::string goldenDir = argv[1], outDir = argv[2];
    for (const PinScenes::Case& c : PinScenes::cases()) {
        if (argc == 4 && std::string(argv[3]) != c.name)
            continue;
        if (!renderCase(c, goldenDir, outDir + "/" + c.name + ".npy"))
            return 1;
    }
    return (argc == 4 || answerHitVectors(goldenDir, outDir + "/vectors")) ? 0 : 1;
}

#endif
