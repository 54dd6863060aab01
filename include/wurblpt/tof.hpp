/*
 * tof.hpp -- the amplitude-modulated continuous-wave (AMCW) time-of-flight camera: LightTof (reference light_tof.hpp:35-69),
 * SensorTofAmcw (sensor_tof_amcw.hpp:50-268) with the reference's public members, defaults and helpers, the two constants
 * they need (constants.hpp:34,38) and mcpt() for the sensor.
 *
 * Not included by wurblpt.hpp: an application includes it next to that header.  The sensor's accumulateRadiance() runs in
 * the HIP kernels (wpt_tof.h behind wpt_render_tof_block of wurblpt_hip.h).  A pixel's paths depend on its index only, so
 * the phase images of one exposure interval trace the same paths; besides the reference's mcpt(sensor, ...), which renders
 * the phase image chosen with setPhaseIndex(), there is an mcpt() that renders all phaseImageCount of them in one launch,
 * each bit for bit what the one-phase render gives.  One device; there is no CPU fallback.
 */
#pragma once

#include <cassert>
#include <cmath>
#include <random>
#include <string>
#include <vector>

#include "wurblpt.hpp"

namespace WurblPT {

inline constexpr double speedOfLight = 299792458.0; /* vacuum, m/s */
inline constexpr float hc = 1.98644582f;            /* Planck's constant times c, in units of 1e-25 J m */

/* light_tof.hpp:45-69: emits (0, 0, 0, radiance) -- near infrared only -- on its front side towards directions within half
 * the opening angle of the normal; a texture scales that by its red value.  What a SensorTofAmcw receives from it is
 * modulated (isTofLight).  To the kernels it is a spot light with the flag WPT_MATF_TOF_LIGHT. */
class LightTof final : public Material
{
private:
    const float _radiance;
    const float _cosHalfOpeningAngle;
    const Texture* _tex;

public:
    LightTof(float radiance, float openingAngle, const Texture* tex = nullptr) :
        _radiance(radiance), _cosHalfOpeningAngle(cosf(0.5f * openingAngle)), _tex(tex)
    {
        assert(openingAngle < pi);
    }
    virtual bool describe(wpt_material& out, FlattenContext& ctx) const override
    {
        out = wptEmptyMaterial(WPT_MAT_LIGHT_SPOT);
        out.flags = WPT_MATF_TOF_LIGHT;
        wptSet(out.v[0], vec4(0.0f, 0.0f, 0.0f, _radiance));
        out.f[0] = _cosHalfOpeningAngle;
        return setTex(out, 0, _tex, ctx) && setNormalTex(out, ctx);
    }
};

class SensorTofAmcw final : public Sensor
{
public:
    constexpr static float dutyCycle = 0.5f; /* share of the exposure in which a tap collects */

    /* the sensor's settings: plain public members with the reference's names, units and defaults */
    unsigned int phaseImageCount; /* result() wants a multiple of 4; the device renders up to WPT_TOF_MAX_PHASES */
    float wavelength;             /* nm */
    double modulationFrequency;   /* Hz */
    float exposureTime;           /* us, per phase image */
    float readoutTime;            /* us, per phase image */
    float pauseTime;              /* us, once per frame behind the last phase image */
    float pixelArea;              /* um^2 */
    float contrast;               /* demodulation contrast of a pixel, 0 .. 1 */
    float quantumEfficiency;      /* electrons per photon */
    int maxElectrons;             /* a tap's full well */

private:
    int _phaseImageIndex;
    Array<float> _frame; /* a, b, total */

public:
    SensorTofAmcw(unsigned int width, unsigned int height) :
        phaseImageCount(4), wavelength(880.0f), modulationFrequency(10e6), exposureTime(1000.0f), readoutTime(1000.0f),
        pauseTime(42000.0f), pixelArea(12.0f * 12.0f), contrast(0.75f), quantumEfficiency(0.8f), maxElectrons(100000),
        _phaseImageIndex(0), _frame(width, height, 3)
    {
    }

    void setPhaseIndex(int i) { _phaseImageIndex = i; }
    int phaseIndex() const { return _phaseImageIndex; }

    float tau(unsigned int phaseImageIndex) const { return phaseImageIndex * (2.0f * pi) / phaseImageCount; }
    /* f / c and c / f: divided as doubles, rounded to float once */
    float fracModfreqC() const { return modulationFrequency / speedOfLight; }
    float fracCModfreq() const { return speedOfLight / modulationFrequency; }

    void setPauseTimeForFPS(float fps)
    {
        const float frame = 1e6f / fps; /* us */
        const float phaseImages = phaseImageCount * (exposureTime + readoutTime);
        pauseTime = frame - phaseImages;
    }
    float frameDuration() const { return (phaseImageCount * (exposureTime + readoutTime) + pauseTime) / 1e6f; }
    float fps() const { return 1.0f / frameDuration(); }
    float phaseImageDuration() const { return (exposureTime + readoutTime) / 1e6f; } /* in seconds */

    /* the record the device path takes: all phases, or the one phase `only` */
    wpt_tof_sensor describe(int only = -1) const
    {
        wpt_tof_sensor s = {};
        s.pixel_area = pixelArea;
        s.exposure_time = exposureTime;
        s.contrast = contrast;
        s.frac_modfreq_c = fracModfreqC();
        s.phase_count = only >= 0 ? 1u : phaseImageCount;
        for (unsigned int j = 0; j < s.phase_count && j < WPT_TOF_MAX_PHASES; j++)
            s.tau[j] = tau(only >= 0 ? (unsigned int)only : j);
        return s;
    }

    /* the energies (a, b, total) of the phase image rendered last by mcpt(sensor, ...) */
    const Array<float>& energy() const { return _frame; }

    /* sensor_tof_amcw.hpp:149-171: energies to the taps' digital numbers (a-b, a+b, a, b) with approximated shot noise */
    Array<float> phase(const Array<float>& energies, float shotNoiseFactor, unsigned long long prngSeed = 42) const
    {
        std::mt19937_64 generator(prngSeed);
        std::normal_distribution<float> gaussianDistribution(0.0f, 1.0f);
        Array<float> phaseImage(energies.dimension(0), energies.dimension(1), 4);
        phaseImage.globalTagList() = energies.globalTagList();
        const float maxElectronsF = maxElectrons;
        for (size_t i = 0; i < phaseImage.elementCount(); i++) {
            float digNums[2];
            /* the reference's vec2 arithmetic, per component.  This port's choice: the first Gaussian draw is tap a's.  The
             * reference draws both inside one constructor call, vec2(g(gen), g(gen)), whose evaluation order C++ leaves open, so
             * which tap gets the first draw there depends on the compiler; with shotNoiseFactor = 0 the images agree either way */
            for (int tap = 0; tap < 2; tap++) {
                /* photons = energy * wavelength / (h c): nm * zJ / (1e-25 J m) leaves a factor 1e-5, half of it in hc's unit */
                float electrons = quantumEfficiency * wavelength * energies[i][tap] / hc / 10000.0f;
                const float shotNoise = std::sqrt(electrons) * gaussianDistribution(generator); /* Gaussian stand-in for Poisson */
                electrons += shotNoiseFactor * shotNoise;
                digNums[tap] = clamp(electrons, 0.0f, maxElectronsF) / maxElectronsF; /* full well = 1 */
            }
            float* out = phaseImage[i];
            out[0] = digNums[0] - digNums[1];
            out[1] = digNums[0] + digNums[1];
            out[2] = digNums[0];
            out[3] = digNums[1];
        }
        return phaseImage;
    }
    Array<float> phase(float shotNoiseFactor, unsigned long long prngSeed = 42) const { return phase(_frame, shotNoiseFactor, prngSeed); }

    /* sensor_tof_amcw.hpp:173-213: distance, amplitude, intensity and phase shift from phaseImageCount phase images (their
     * component 0, a-b, is what counts); all but the intensity's and amplitude's scale are invariant to the images' scale */
    Array<float> result(const Array<float>* phases) const
    {
        assert(phaseImageCount % 4 == 0);
        const unsigned int quarter = phaseImageCount / 4; /* the images at 0, 90, 180 and 270 degrees */
        Array<float> r(phases[0].dimension(0), phases[0].dimension(1), 4);
        r.globalTagList() = phases[0].globalTagList();
        for (size_t i = 0; i < r.elementCount(); i++) {
            const float d0 = phases[0][i][0], d90 = phases[quarter][i][0], d180 = phases[2 * quarter][i][0], d270 = phases[3 * quarter][i][0];
            float shift = 0.0f, distance = 0.0f;
            if (!(std::fabs(d0 - d180) <= 0.0f && std::fabs(d90 - d270) <= 0.0f)) {
                shift = atan(d270 - d90, d0 - d180);
                if (shift < 0.0f)
                    shift += 2.0 * pi; /* (a double sum, rounded to float) */
                distance = fracCModfreq() * shift * 0.25f * inv_pi;
            }
            float* out = r[i];
            out[0] = distance;
            out[1] = std::sqrt((d0 - d180) * (d0 - d180) + (d90 - d270) * (d90 - d270)) * pi_2; /* amplitude */
            out[2] = 0.5f * (d0 + d90 + d180 + d270);                                            /* intensity */
            out[3] = shift;
        }
        return r;
    }

    virtual unsigned int width() const override { return _frame.dimension(0); }
    virtual unsigned int height() const override { return _frame.dimension(1); }
    virtual ArrayContainer* pixelArray() override { return &_frame; }
};

/* renders the phase images of `record` (phase_count planes of a, b, total) into `planes`, one launch */
inline void mcptTofPlanes(float* planes, const wpt_tof_sensor& record, std::vector<ArrayContainer*> tagged, unsigned int width,
        unsigned int height, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0, float t1, const Parameters& params)
{
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
    wpt_params p = makeParams(params, SensorRGB(1, 1)); /* the default gates: the sensor has none */
    p.t0 = t0;
    p.t1 = t1;
    fprintf(stderr, "Number of hitables that are hot spots: %zu\n", scene.hotSpots().size());
    fprintf(stderr, "Rendering %ux%u pixels with %u samples into %u time-of-flight phase image(s).\n", width, height,
            samplesSqrt * samplesSqrt, record.phase_count);
    if (wpt_device_count() <= 0)
        mcptFatal(std::string("no HIP device: ") + wpt_last_error());
    const auto renderStart = std::chrono::steady_clock::now();
    wpt_scene* dscene = nullptr;
    if (wpt_scene_upload(&desc, &dscene) != WPT_OK)
        mcptFatal(wpt_last_error());
    const wpt_status st = wpt_render_tof_block(dscene, &cam, &p, &record, width, height, samplesSqrt, 0, width * height, planes);
    const std::string renderError = st == WPT_OK ? "" : wpt_last_error();
    wpt_scene_free(dscene);
    if (st != WPT_OK)
        mcptFatal(renderError);
    int device = 0;
    if (wpt_current_device(&device) != WPT_OK)
        device = 0;
    const std::string seconds = std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count());
    for (ArrayContainer* a : tagged) {
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

/* the reference's mcpt() for this sensor: the phase image set with setPhaseIndex(), into sensor.energy() */
inline void mcpt(SensorTofAmcw& sensor, const Camera& camera, const Scene& scene, unsigned int samplesSqrt, float t0 = 0.0f,
        float t1 = 0.0f, const Parameters& params = Parameters())
{
    ArrayContainer* frame = sensor.pixelArray();
    mcptTofPlanes(static_cast<float*>(frame->data()), sensor.describe(sensor.phaseIndex()), { frame }, sensor.width(), sensor.height(),
            camera, scene, samplesSqrt, t0, t1, params);
    frame->globalTagList().set("WURBLPT/TOF_PHASE_INDEX", std::to_string(sensor.phaseIndex()));
}

/* this port's addition: all sensor.phaseImageCount phase images of the exposure interval [t0, t1] in one launch;
 * energies[j] is bit for bit what mcpt(sensor, ...) gives after setPhaseIndex(j) */
inline void mcpt(std::vector<Array<float>>& energies, SensorTofAmcw& sensor, const Camera& camera, const Scene& scene,
        unsigned int samplesSqrt, float t0 = 0.0f, float t1 = 0.0f, const Parameters& params = Parameters())
{
    const unsigned int n = sensor.phaseImageCount;
    if (n == 0 || n > WPT_TOF_MAX_PHASES)
        mcptFatal("SensorTofAmcw: the device path renders 1 .. " + std::to_string(WPT_TOF_MAX_PHASES) + " phase images");
    const size_t planeFloats = size_t(sensor.width()) * sensor.height() * 3;
    std::vector<float> planes(planeFloats * n);
    energies.clear();
    std::vector<ArrayContainer*> tagged;
    for (unsigned int j = 0; j < n; j++)
        energies.emplace_back(sensor.width(), sensor.height(), 3);
    for (unsigned int j = 0; j < n; j++)
        tagged.push_back(&energies[j]);
    mcptTofPlanes(planes.data(), sensor.describe(), tagged, sensor.width(), sensor.height(), camera, scene, samplesSqrt, t0, t1, params);
    for (unsigned int j = 0; j < n; j++) {
        std::copy(planes.begin() + j * planeFloats, planes.begin() + (j + 1) * planeFloats, static_cast<float*>(energies[j].data()));
        energies[j].globalTagList().set("WURBLPT/TOF_PHASE_INDEX", std::to_string(j));
    }
}

}
