/*
 * ref_frames.cpp -- renders the cases of pin_scenes.hpp with THE REFERENCE'S OWN mcpt().
 *
 * TEST INFRASTRUCTURE.  Compiled only where the reference tree exists, by oracle/Makefile, against
 * the reference's headers where they lie and the container stand-in oracle/tgd_standin/ (the
 * reference's library wants an external container library that is not installed; the stand-in is
 * this repository's own text).  The binary goes to oracle/_ref/ (git-ignored); what it writes
 * -- frames, time-of-flight energies and vectors of the reference's own classes, as float32 data --
 * goes to tests/golden/frames/ and is committed: data only, no reference source.
 *
 *   ref_frames <tests/golden> <output directory> [one case]
 *
 * One thread renders (OMP_NUM_THREADS is not consulted: the thread count is set here), so a
 * frame does not depend on the machine.  A pixel's samples depend on the pixel alone anyway.
 */
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include <omp.h>

/* the two libraries that the reference keeps in a source file of their own */
#define POWITACQ_IMPLEMENTATION
#define TINYOBJLOADER_IMPLEMENTATION
#include "wurblpt.hpp"

template<typename T> TGD::Array<T> pinArray(size_t width, size_t height, size_t components)
{
    return TGD::Array<T>({ width, height }, components);
}

#include "pin_scenes.hpp"
#include "pin_io.hpp"

using namespace WurblPT;

/* SensorTofAmcw::accumulateRadiance over seeded (radiance, optical path length, ToF light or not, phase): rows of
 * [radiance.w, opl.w, isTofLight, phase, a, b, total].  The hit record points at a triangle whose material is a LightTof or a
 * LightDiffuse, which is all that accumulateRadiance asks of it. */
static std::vector<float> tofVectors(size_t n)
{
    Scene scene;
    Material* tofLight = scene.take(new LightTof(1.0f, radians(120.0f)));
    Material* plain = scene.take(new LightDiffuse(vec4(1.0f)));
    std::vector<const Hitable*> a = scene.take(new MeshInstance(scene.take(generateQuad()), tofLight));
    std::vector<const Hitable*> b = scene.take(new MeshInstance(scene.take(generateQuad()), plain));
    SensorTofAmcw sensor(1, 1);
    Prng prng(4711);
    std::vector<float> rows;
    for (size_t i = 0; i < n; i++) {
        const float radiance = (i % 7 == 0) ? 0.0f : 50.0f * prng.in01() * prng.in01();
        const float opl = (i % 11 == 0) ? 0.0f : 40.0f * prng.in01();
        const int isTof = prng.in01() < 0.7f ? 1 : 0;
        const int phase = int(i % 4);
        HitRecord hr(1.0f);
        hr.haveHit = true;
        hr.hitable = isTof ? a[0] : b[0];
        hr.backside = false;
        hr.normal = vec3(0.0f, 0.0f, 1.0f);
        float acc[3] = { 0.0f, 0.0f, 0.0f };
        sensor.setPhaseIndex(phase);
        sensor.accumulateRadiance(Ray(vec3(0.0f), vec3(0.0f, 0.0f, -1.0f), 0.0f, vec4(1.0f)), 2, opl, vec4(opl), 1.0f, vec4(0.0f, 0.0f, 0.0f, radiance), hr, 0.0f, 0.0f, acc);
        const float row[7] = { radiance, opl, float(isTof), float(phase), acc[0], acc[1], acc[2] };
        rows.insert(rows.end(), row, row + 7);
    }
    return rows;
}

/* ---- vectors of the reference's own classes, in the layouts of the restatement's probes (wpt_oracle.cpp: wpt_oracle_bvh_hits,
 * wpt_oracle_hotspot_probe, wpt_oracle_material_probe, wpt_oracle_envmap_probe): every row is the probe's input record followed
 * by what the reference answers ---- */

static vec3 unitVector(Prng& g)
{
    const float z = 2.0f * g.in01() - 1.0f, phi = 2.0f * pi * g.in01(), r = sqrt(max(0.0f, 1.0f - z * z));
    return normalize(vec3(r * cos(phi), r * sin(phi), z));
}

static void push(std::vector<float>& rows, const vec3& v) { rows.push_back(v.x()); rows.push_back(v.y()); rows.push_back(v.z()); }
static void push(std::vector<float>& rows, const vec4& v) { rows.push_back(v.x()); rows.push_back(v.y()); rows.push_back(v.z()); rows.push_back(v.w()); }

/* rows of 1 + 18 + 22: Scene::materialIndex() | ray direction, hit normal, hit tangent, texcoords, backside, a, seed, direction
 * to evaluate, refractive index of the ray | scatter (type, direction, attenuation, pdf, refractive index), scatterToDirection
 * (attenuation, pdf), emitted */
static std::vector<float> materialVectors(const std::string& goldenDir, size_t perMaterial)
{
    PinScenes::Setup s;
    s.width = 32;
    s.height = 24;
    s.goldenDir = goldenDir;
    std::vector<const Material*> list;
    PinScenes::materialsForProbe(s, list);
    std::vector<float> rows;
    for (size_t m = 0; m < list.size(); m++) {
        Prng g(1000 + m);
        for (size_t i = 0; i < perMaterial; i++) {
            const vec3 n = unitVector(g);
            vec3 other = unitVector(g);
            while (abs(dot(other, n)) > 0.9f)
                other = unitVector(g);
            const vec3 tangent = normalize(cross(n, other));
            /* the record's normal faces the ray; every second ray comes in near the normal, where the spot lights' cones are */
            vec3 d = (i % 4 == 1) ? normalize(-n + 0.2f * unitVector(g)) : (i % 4 == 3) ? normalize(-n + 0.6f * unitVector(g)) : unitVector(g);
            if (dot(n, d) > 0.0f)
                d = -d;
            if (dot(n, d) > -0.02f)
                d = normalize(d - 0.1f * n);
            const vec2 tc(g.in01(), g.in01());
            const bool backside = g.in01() < 0.3f;
            const float a = 0.5f + 3.0f * g.in01();
            const float seed = float(int(g.in01() * 60000.0f));
            const vec3 e = unitVector(g);
            const float refr = g.in01() < 0.3f ? 1.5f : 1.0f;
            const Ray ray(vec3(0.0f), d, 0.0f, vec4(refr));
            const HitRecord hit(a, ray.at(a), n, tangent, tc, backside, nullptr);
            Prng prng(static_cast<unsigned int>(seed));
            const ScatterRecord sr = list[m]->scatter(ray, hit, prng);
            const ScatterRecord ev = list[m]->scatterToDirection(ray, hit, e);
            const vec4 em = list[m]->emitted(ray, hit);
            rows.push_back(float(s.scene.materialIndex(list[m])));
            push(rows, d); push(rows, n); push(rows, tangent);
            rows.push_back(tc.x()); rows.push_back(tc.y());
            rows.push_back(backside ? 1.0f : 0.0f); rows.push_back(a); rows.push_back(seed);
            push(rows, e);
            rows.push_back(refr);
            rows.push_back(float(sr.type));
            push(rows, sr.direction); push(rows, sr.attenuation); rows.push_back(sr.pdf); push(rows, sr.refractiveIndex);
            push(rows, ev.attenuation); rows.push_back(ev.pdf);
            push(rows, em);
        }
    }
    return rows;
}

/* rows of 8 + 15: origin, direction, amin, amax | haveHit, (unused: the restatement's index of the triangle), a, position,
 * normal, tangent, texcoords, backside; Scene::bvh().hit, which asks HitableTriangle::hit at the leaves */
static std::vector<float> hitVectors(const PinScenes::Case& c, PinScenes::Setup& s)
{
    std::vector<std::pair<vec3, vec3>> rays; /* origin, target */
    Prng g(77);
    if (std::string(c.name) == "cornell") {
        /* the room is [-1,1]^3 without a front; floor in 3x3 cells, ceiling and back wall in 2x2, each cell two triangles */
        const vec3 eye(0.0f, 0.0f, 3.7f), inside(0.3f, -0.2f, 0.4f);
        const float third = 1.0f / 3.0f;
        std::vector<vec3> targets;
        for (int k = 0; k <= 8; k++) {
            const float u = -1.0f + k / 4.0f;
            targets.push_back(vec3(-1.0f, u, -1.0f));  /* back wall / left wall */
            targets.push_back(vec3(1.0f, u, -1.0f));   /* back wall / right wall */
            targets.push_back(vec3(u, -1.0f, -1.0f));  /* back wall / floor */
            targets.push_back(vec3(u, 1.0f, -1.0f));   /* back wall / ceiling */
            targets.push_back(vec3(-1.0f, -1.0f, u));  /* floor / left wall */
            targets.push_back(vec3(1.0f, 1.0f, u));    /* ceiling / right wall */
            targets.push_back(vec3(-third, -1.0f, u)); /* floor, between cells */
            targets.push_back(vec3(u, -1.0f, third));
            targets.push_back(vec3(u, -1.0f, u));      /* floor, a cell's diagonal (one of the two it may have) */
            targets.push_back(vec3(u, -1.0f, -u));
            targets.push_back(vec3(0.0f, u, -1.0f));   /* back wall, between cells */
            targets.push_back(vec3(u, u, -1.0f));
            targets.push_back(vec3(u, -u, -1.0f));
            targets.push_back(vec3(0.25f * u, 1.0f, 0.25f)); /* the lamp's edge in the ceiling plane */
        }
        for (const vec3& tgt : targets) {
            const vec3 origins[2] = { eye, inside };
            for (int o = 0; o < 2; o++) {
                const vec3& from = origins[o];
                rays.push_back({ from, tgt });
                /* and, from the camera, one step of the target to either side in every coordinate */
                for (int axis = 0; axis < 3 && o == 0; axis++) {
                    vec3 lo = tgt, hi = tgt;
                    lo[axis] = std::nextafter(tgt[axis], -2.0f);
                    hi[axis] = std::nextafter(tgt[axis], 2.0f);
                    rays.push_back({ from, lo });
                    rays.push_back({ from, hi });
                }
            }
        }
        /* parallel incidence: rays that travel inside the planes of the floor, the ceiling and a wall */
        for (int k = 0; k < 24; k++) {
            const float u = -0.9f + 0.075f * k;
            rays.push_back({ vec3(u, -1.0f, 3.0f), vec3(u, -1.0f, -1.0f) });
            rays.push_back({ vec3(u, 1.0f, 3.0f), vec3(-u, 1.0f, -1.0f) });
            rays.push_back({ vec3(-1.0f, u, 3.0f), vec3(-1.0f, -u, -1.0f) });
            rays.push_back({ vec3(0.5f, 1.0f, 0.5f), vec3(u, 1.0f, -u) }); /* from the ceiling plane along it, as the lamp's light rays go */
            rays.push_back({ vec3(3.0f * u, 2.5f, -3.0f), vec3(u, -u, 0.0f) }); /* from outside: the walls' back sides */
        }
    } else {
        const vec3 eye(0.0f, 1.3f, 4.2f);
        for (int k = 0; k < 600; k++)
            rays.push_back({ (k % 6 == 5) ? vec3(6.0f * g.in01() - 3.0f, -2.0f, -4.0f) : eye, /* every sixth from below and behind */
                    vec3(-2.5f + 5.0f * g.in01(), 3.0f * g.in01(), -2.0f + 3.0f * g.in01()) });
    }
    AnimationCache cache(s.scene.animations(), c.t0);
    std::vector<float> rows;
    for (const auto& r : rays) {
        const vec3 d = normalize(r.second - r.first);
        const float amin = s.params.minHitDistance, amax = maxval;
        const Ray ray(r.first, d, c.t0, vec4(1.0f));
        Prng prng(1);
        const HitRecord hr = s.scene.bvh().hit(ray, RayIntersectionHelper(ray), amin, amax, amin, cache, prng);
        push(rows, r.first); push(rows, d);
        rows.push_back(amin); rows.push_back(amax);
        rows.push_back(hr.haveHit ? 1.0f : 0.0f);
        rows.push_back(0.0f);
        if (hr.haveHit) {
            rows.push_back(hr.a);
            push(rows, hr.position); push(rows, hr.normal); push(rows, hr.tangent);
            rows.push_back(hr.texcoords.x()); rows.push_back(hr.texcoords.y());
            rows.push_back(hr.backside ? 1.0f : 0.0f);
        } else {
            rows.insert(rows.end(), 13, 0.0f);
        }
    }
    return rows;
}

/* rows of 7 + 7: origin, a direction, seed | the light sampling of tracePath with Hitable::pdfValue and Hitable::direction */
static std::vector<float> hotSpotVectors(const PinScenes::Case& c, PinScenes::Setup& s, size_t n)
{
    const std::vector<const Hitable*>& hotSpots = s.scene.hotSpots();
    const size_t hotSpotsSize = hotSpots.size();
    const float invHotSpotsSize = 1.0f / hotSpotsSize;
    AnimationCache cache(s.scene.animations(), c.t0);
    Prng g(4242);
    std::vector<float> rows;
    for (size_t i = 0; i < n; i++) {
        const vec3 origin(-2.0f + 4.0f * g.in01(), 0.1f + 1.9f * g.in01(), -1.5f + 3.5f * g.in01());
        /* two of three directions point at a hot spot, where the densities are not zero */
        vec3 direction = unitVector(g);
        if (i % 3 != 0) {
            size_t k = g.in01() * hotSpotsSize;
            direction = hotSpots[min(k, hotSpotsSize - 1)]->direction(origin, cache, g);
        }
        const float seed = float(int(g.in01() * 60000.0f));
        Prng prng(static_cast<unsigned int>(seed));
        float hotSpotsPdf = 0.0f;
        for (size_t k = 0; k < hotSpotsSize; k++)
            hotSpotsPdf += hotSpots[k]->pdfValue(origin, direction, cache, prng);
        hotSpotsPdf *= invHotSpotsSize;
        size_t hotSpotIndex = prng.in01() * hotSpotsSize;
        hotSpotIndex = min(hotSpotIndex, hotSpotsSize - 1);
        const vec3 directDir = hotSpots[hotSpotIndex]->direction(origin, cache, prng);
        float directPdf = 0.0f;
        for (size_t k = 0; k < hotSpotsSize; k++)
            directPdf += hotSpots[k]->pdfValue(origin, directDir, cache, prng);
        directPdf *= invHotSpotsSize;
        push(rows, origin); push(rows, direction); rows.push_back(seed);
        rows.push_back(hotSpotsPdf); rows.push_back(float(hotSpotIndex));
        push(rows, directDir);
        rows.push_back(directPdf);
        rows.push_back(hotSpots[0]->pdfValue(origin, direction, cache, prng));
    }
    return rows;
}

/* rows of 4 + 10: direction, seed | L(direction), p(direction), d(prng), p(d), the sum of L(d)'s channels; an environment map
 * with importance sampling */
static std::vector<float> envmapVectors(PinScenes::Setup& s, size_t n)
{
    const EnvironmentMap* env = s.scene.environmentMap();
    Prng g(99);
    std::vector<float> rows;
    for (size_t i = 0; i < n; i++) {
        const vec3 direction = unitVector(g);
        const float seed = float(int(g.in01() * 60000.0f));
        Prng prng(static_cast<unsigned int>(seed));
        const vec4 L = env->L(direction);
        const float p = env->p(direction);
        const vec3 d = env->d(prng);
        const float pd = env->p(d);
        const vec4 Ld = env->L(d);
        push(rows, direction); rows.push_back(seed);
        push(rows, L); rows.push_back(p); push(rows, d); rows.push_back(pd);
        rows.push_back(Ld.x() + Ld.y() + Ld.z() + Ld.w());
    }
    return rows;
}

int main(int argc, char* argv[])
{
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s <tests/golden> <output directory> [one case]\n", argv[0]);
        return 2;
    }
    const std::string goldenDir = argv[1], outDir = argv[2];
    omp_set_num_threads(1);
    std::string index = "{\n\"generator\": \"oracle/ref_frames.cpp: the reference's mcpt() over oracle/pin_scenes.hpp\",\n\"cases\": [\n";
    bool first = true;
    for (const PinScenes::Case& c : PinScenes::cases()) {
        if (argc == 4 && std::string(argv[3]) != c.name)
            continue;
        PinScenes::Setup s;
        PinScenes::setUp(c, s, goldenDir);
        std::vector<float> data;
        std::vector<size_t> shape;
        if (c.tof) {
            SensorTofAmcw sensor(c.width, c.height);
            for (unsigned int j = 0; j < sensor.phaseImageCount; j++) {
                sensor.setPhaseIndex(j);
                mcpt(sensor, *s.camera, s.scene, c.samplesSqrt, c.t0, c.t1, s.params);
                const float* e = static_cast<const float*>(sensor.energy().data());
                data.insert(data.end(), e, e + size_t(c.width) * c.height * 3);
            }
            shape = { sensor.phaseImageCount, c.height, c.width, 3 };
        } else {
            SensorRGB sensor(c.width, c.height, s.minDistToLight, s.maxDistToLight, s.minPathLen, s.maxPathLen);
            mcpt(sensor, *s.camera, s.scene, c.samplesSqrt, c.t0, c.t1, s.params);
            const float* f = static_cast<const float*>(sensor.result().data());
            data.assign(f, f + size_t(c.width) * c.height * 3);
            shape = { c.height, c.width, 3 };
        }
        if (!PinIO::writeNpy(outDir + "/" + c.name + ".npy", shape, data.data())) {
            fprintf(stderr, "cannot write %s/%s.npy\n", outDir.c_str(), c.name);
            return 1;
        }
        char line[512];
        snprintf(line, sizeof(line), "%s{\"name\": \"%s\", \"width\": %u, \"height\": %u, \"samples_sqrt\": %u, \"tof\": %s, \"features\": %s, \"unlike\": %s}",
                first ? "" : ",\n", c.name, c.width, c.height, c.samplesSqrt, c.tof ? "true" : "false",
                PinIO::jsonList(c.features).c_str(), PinIO::jsonList(c.unlike).c_str());
        index += line;
        first = false;
    }
    index += "\n]\n}\n";

    if (argc == 4)
        return 0; /* one case for a look at it: neither the index nor the vectors */

    const std::vector<float> tof = tofVectors(512);
    if (!PinIO::writeNpy(outDir + "/vectors_tof_accumulate.npy", { tof.size() / 7, 7 }, tof.data()))
        return 1;
    const std::vector<float> materials = materialVectors(goldenDir, 32);
    if (!PinIO::writeNpy(outDir + "/vectors_materials.npy", { materials.size() / 41, 41 }, materials.data()))
        return 1;
    for (const PinScenes::Probe& probe : PinScenes::probes()) {
        const PinScenes::Case& c = *PinScenes::findCase(probe.caseName);
        PinScenes::Setup s;
        PinScenes::setUp(c, s, goldenDir);
        const std::string kind = probe.kind;
        const std::vector<float> rows = kind == "hits" ? hitVectors(c, s) : kind == "hotspots" ? hotSpotVectors(c, s, 256) : envmapVectors(s, 256);
        const size_t width = kind == "hits" ? 23 : 14;
        if (!PinIO::writeNpy(outDir + "/vectors_" + kind + "_" + c.name + ".npy", { rows.size() / width, width }, rows.data()))
            return 1;
    }

    FILE* f = fopen((outDir + "/index.json").c_str(), "wb");
    if (!f || fwrite(index.data(), 1, index.size(), f) != index.size() || fclose(f) != 0)
        return 1;
    return 0;
}
