/*
 * pin_scenes.hpp -- TEST INFRASTRUCTURE: the scenes of the reference-frame pin, written once and
 * compiled twice: by oracle/ref_frames.cpp against the reference's headers (its mcpt() renders
 * the committed fixtures tests/golden/frames/) and by oracle/pin_render.cpp against include/
 * (the restatement and the product render the same cases and must give the same bits).
 *
 * This file includes nothing.  Its includer has already included the umbrella header of the
 * header set it chose (and <memory>, <string>, <vector>, <limits>; of include/ also wurblpt/tof.hpp, which
 * that set keeps beside its umbrella header, for LightTof and SensorTofAmcw), and provides
 *     template<typename T> TGD::Array<T> pinArray(size_t width, size_t height, size_t components);
 * because the two containers spell that constructor differently.  Everything else here is API
 * that both header sets share.
 *
 * A case builds a Scene, a Camera, Parameters and the sensor's gates; the table at the end names
 * the cases, their frame size, samples, exposure interval and the features they carry.
 */
#pragma once

namespace PinScenes {

using namespace WurblPT;

struct Setup
{
    unsigned int width, height;
    std::string goldenDir; /* where tests/golden/ lies (the RGL fixtures) */
    Scene scene;
    std::unique_ptr<Camera> camera;
    Parameters params;
    float minDistToLight = 0.0f, maxDistToLight = std::numeric_limits<float>::max();
    float minPathLen = 0.0f, maxPathLen = std::numeric_limits<float>::max();
    float aspect() const { return float(width) / height; }
};

struct Case
{
    const char* name;
    void (*build)(Setup&);
    unsigned int width, height, samplesSqrt;
    float t0, t1;
    bool tof;             /* SensorTofAmcw, all four phase images; otherwise SensorRGB */
    const char* features; /* space separated, for the index */
    const char* unlike;   /* space separated names of cases whose frame must differ from this one's */
};

/* ---- building blocks ---- */

inline const quat faceUp() { return toQuat(radians(-90.0f), vec3(1.0f, 0.0f, 0.0f)); }
inline const quat faceDown() { return toQuat(radians(90.0f), vec3(1.0f, 0.0f, 0.0f)); }

inline void standardCamera(Setup& s, const Optics* optics = nullptr)
{
    const Optics o = optics ? *optics : Optics(Projection(radians(50.0f), s.aspect()));
    s.camera.reset(new Camera(o, Transformation::fromLookAt(vec3(0.0f, 1.3f, 4.2f), vec3(0.0f, 0.9f, 0.0f))));
}

/* a floor, a back wall and two coloured side walls; generateQuad() is [-1,1]^2 in the xy plane facing +z */
inline void room(Setup& s, Material* floor = nullptr)
{
    Scene& sc = s.scene;
    if (!floor)
        floor = sc.take(new MaterialLambertian(vec3(0.7f)));
    Material* back = sc.take(new MaterialLambertian(vec3(0.6f, 0.6f, 0.65f)));
    Material* left = sc.take(new MaterialLambertian(vec3(0.65f, 0.1f, 0.08f)));
    Material* right = sc.take(new MaterialLambertian(vec3(0.1f, 0.5f, 0.12f)));
    sc.take(new MeshInstance(sc.take(generateQuad()), floor, Transformation(vec3(0.0f), faceUp(), vec3(3.0f, 3.0f, 1.0f))));
    sc.take(new MeshInstance(sc.take(generateQuad()), back, Transformation(vec3(0.0f, 1.5f, -2.0f), quat::null(), vec3(3.0f, 1.5f, 1.0f))));
    sc.take(new MeshInstance(sc.take(generateQuad()), left,
                Transformation(vec3(-2.5f, 1.5f, 0.0f), toQuat(radians(90.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(3.0f, 1.5f, 1.0f))));
    sc.take(new MeshInstance(sc.take(generateQuad()), right,
                Transformation(vec3(2.5f, 1.5f, 0.0f), toQuat(radians(-90.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(3.0f, 1.5f, 1.0f))));
}

inline void ceilingLight(Setup& s, const vec3& emit = vec3(9.0f), float size = 0.6f, const vec3& at = vec3(0.0f, 2.8f, 0.3f))
{
    Material* light = s.scene.take(new LightDiffuse(emit));
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), light, Transformation(at, faceDown(), vec3(size))), HotSpot);
}

inline void cube(Setup& s, Material* m, const vec3& at, float size, float turn = 25.0f)
{
    s.scene.take(new MeshInstance(s.scene.take(generateCube()), m,
                Transformation(at, toQuat(radians(turn), vec3(0.0f, 1.0f, 0.0f)), vec3(size))));
}

/* deterministic texel values in [0, 1): an integer hash of the position */
inline float texel01(unsigned int x, unsigned int y, unsigned int c)
{
    unsigned int h = (x * 73856093u) ^ (y * 19349663u) ^ (c * 83492791u);
    h ^= h >> 13;
    h *= 0x5bd1e995u;
    h ^= h >> 15;
    return (h & 0xffffu) / 65536.0f;
}

template<typename T> inline Texture* imageTexture(Setup& s, unsigned int w, unsigned int h, unsigned int comps, float scale, float bias,
        LinearizeSRGBType lin = LinearizeSRGB_Auto)
{
    auto img = pinArray<T>(w, h, comps);
    for (unsigned int y = 0; y < h; y++)
        for (unsigned int x = 0; x < w; x++)
            for (unsigned int c = 0; c < comps; c++)
                img[y * w + x][c] = T(bias + scale * texel01(x, y, c));
    return s.scene.take(createTextureImage(img, lin));
}

/* ---- materials, one by one, in the room ---- */

inline void lambertian(Setup& s)
{
    room(s);
    ceilingLight(s);
    cube(s, s.scene.take(new MaterialLambertian(vec3(0.3f, 0.4f, 0.8f))), vec3(-0.9f, 0.5f, 0.2f), 0.5f);
    cube(s, s.scene.take(new MaterialLambertian(vec3(0.8f, 0.7f, 0.2f))), vec3(0.9f, 0.35f, 0.6f), 0.35f, -20.0f);
    standardCamera(s);
}

inline void ggx(Setup& s)
{
    Texture* rough = s.scene.take(new TextureChecker(vec3(0.05f, 0.3f, 0.0f), vec3(0.4f, 0.1f, 0.0f), 5, 5));
    room(s, s.scene.take(new MaterialGGX(vec3(0.8f, 0.8f, 0.75f), vec2(0.2f, 0.2f), nullptr, rough)));
    ceilingLight(s);
    cube(s, s.scene.take(new MaterialGGX(vec3(0.9f, 0.6f, 0.3f), vec2(0.05f, 0.35f))), vec3(-0.9f, 0.5f, 0.2f), 0.5f);
    cube(s, s.scene.take(new MaterialGGX(vec3(0.7f, 0.75f, 0.9f), vec2(0.3f, 0.08f))), vec3(0.9f, 0.35f, 0.6f), 0.35f, -20.0f);
    standardCamera(s);
}

inline void glass(Setup& s)
{
    room(s);
    ceilingLight(s);
    cube(s, s.scene.take(new MaterialGlass(vec3(0.0f), 1.5f)), vec3(-0.9f, 0.5f, 0.4f), 0.5f);
    cube(s, s.scene.take(new MaterialGlass(vec3(0.9f, 0.2f, 0.4f), vec3(1.45f, 1.5f, 1.58f))), vec3(0.9f, 0.45f, 0.6f), 0.45f, -20.0f);
    standardCamera(s);
}

inline void mirror(Setup& s)
{
    room(s);
    ceilingLight(s);
    cube(s, s.scene.take(new MaterialMirror(vec3(0.95f, 0.9f, 0.8f))), vec3(-0.9f, 0.5f, 0.2f), 0.5f);
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), s.scene.take(new MaterialMirror()),
                Transformation(vec3(1.2f, 1.0f, -1.2f), toQuat(radians(-35.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.9f, 0.8f, 1.0f))));
    standardCamera(s);
}

inline void modphong(Setup& s)
{
    Texture* dif = s.scene.take(new TextureChecker(vec3(0.6f, 0.2f, 0.1f), vec3(0.1f, 0.3f, 0.6f), 6, 6));
    room(s, s.scene.take(new MaterialModPhong(vec3(0.5f), dif, vec3(0.3f), nullptr, 60.0f)));
    ceilingLight(s);
    cube(s, s.scene.take(new MaterialModPhong(vec3(0.3f, 0.5f, 0.2f), vec3(0.5f), 120.0f, 0.55f)), vec3(-0.9f, 0.5f, 0.4f), 0.5f);
    cube(s, s.scene.take(new MaterialModPhong(vec3(0.6f, 0.5f, 0.2f), vec3(0.2f), 20.0f)), vec3(0.9f, 0.35f, 0.6f), 0.35f, -20.0f);
    standardCamera(s);
}

inline void twosided(Setup& s)
{
    room(s);
    ceilingLight(s);
    Material* front = s.scene.take(new MaterialModPhong(vec3(0.5f, 0.3f, 0.2f), vec3(0.4f), 80.0f));
    Material* back = s.scene.take(new MaterialGGX(vec3(0.3f, 0.6f, 0.8f), vec2(0.15f, 0.25f)));
    Material* two = s.scene.take(new MaterialTwoSided(front, back));
    /* one quad seen from its front, one from its back */
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), two,
                Transformation(vec3(-1.0f, 0.8f, 0.0f), toQuat(radians(30.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.7f))));
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), two,
                Transformation(vec3(1.0f, 0.8f, 0.0f), toQuat(radians(150.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.7f))));
    standardCamera(s);
}

/* ---- spot lights: one scene, the lamp varies ---- */

inline void spotScene(Setup& s, float angleDegrees, bool textured, bool insideTwoSided)
{
    room(s);
    ceilingLight(s, vec3(3.0f), 0.3f, vec3(-1.6f, 2.8f, 0.8f));
    cube(s, s.scene.take(new MaterialLambertian(vec3(0.7f, 0.7f, 0.3f))), vec3(0.7f, 0.3f, 0.3f), 0.3f);
    if (angleDegrees > 0.0f) {
        Texture* gobo = textured ? s.scene.take(new TextureChecker(vec3(1.0f, 0.9f, 0.8f), vec3(0.05f, 0.1f, 0.3f), 4, 4)) : nullptr;
        Material* lamp = s.scene.take(new LightSpot(radians(angleDegrees), vec3(14.0f, 12.0f, 9.0f), gobo));
        if (insideTwoSided)
            lamp = s.scene.take(new MaterialTwoSided(lamp, s.scene.take(new MaterialLambertian(vec3(0.0f)))));
        /* tilted, so that the cone's edge crosses the floor, a wall and the cube */
        const quat tilt = toQuat(radians(90.0f), vec3(1.0f, 0.0f, 0.0f)) * toQuat(radians(12.0f), vec3(0.0f, 1.0f, 0.0f));
        s.scene.take(new MeshInstance(s.scene.take(generateQuad()), lamp, Transformation(vec3(0.4f, 2.2f, 0.2f), tilt, vec3(0.25f))), HotSpot);
    }
    standardCamera(s);
}
inline void spot30(Setup& s) { spotScene(s, 30.0f, false, false); }
inline void spot70(Setup& s) { spotScene(s, 70.0f, false, false); }
inline void spot360(Setup& s) { spotScene(s, 360.0f, false, false); }
inline void spotNone(Setup& s) { spotScene(s, 0.0f, false, false); }
inline void spot70Textured(Setup& s) { spotScene(s, 70.0f, true, false); }
inline void spot360Textured(Setup& s) { spotScene(s, 360.0f, true, false); }
inline void spot30TwoSided(Setup& s) { spotScene(s, 30.0f, false, true); }
inline void spot360TwoSided(Setup& s) { spotScene(s, 360.0f, false, true); }

/* ---- textures ---- */

inline void textures(Setup& s)
{
    Texture* checker = s.scene.take(new TextureChecker(vec3(0.8f), vec3(0.15f, 0.2f, 0.3f), 7, 5));
    Texture* moved = s.scene.take(new TextureTransformer(checker, vec2(2.0f, 3.0f), vec2(0.13f, 0.29f), vec4(0.8f), vec4(0.1f)));
    room(s, s.scene.take(new MaterialLambertian(vec3(1.0f), moved)));
    ceilingLight(s);
    Texture* srgb8 = imageTexture<uint8_t>(s, 7, 5, 3, 255.0f, 0.0f);
    Texture* grey16 = imageTexture<uint16_t>(s, 5, 6, 1, 65535.0f, 0.0f);
    Texture* rgba32 = imageTexture<float>(s, 6, 4, 4, 0.8f, 0.1f);
    Texture* grey8 = imageTexture<uint8_t>(s, 3, 3, 1, 255.0f, 0.0f, LinearizeSRGB_Off);
    Texture* rgb16 = imageTexture<uint16_t>(s, 4, 7, 3, 65535.0f, 0.0f);
    cube(s, s.scene.take(new MaterialLambertian(vec3(1.0f), srgb8)), vec3(-1.3f, 0.4f, 0.4f), 0.4f);
    cube(s, s.scene.take(new MaterialLambertian(vec3(1.0f), grey16)), vec3(-0.3f, 0.4f, -0.4f), 0.4f, 50.0f);
    cube(s, s.scene.take(new MaterialModPhong(vec4(1.0f), rgba32, vec4(0.0f))), vec3(0.6f, 0.4f, 0.5f), 0.4f, -15.0f);
    cube(s, s.scene.take(new MaterialLambertian(vec3(1.0f), grey8)), vec3(1.5f, 0.3f, -0.3f), 0.3f, 10.0f);
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), s.scene.take(new MaterialLambertian(vec3(1.0f), rgb16)),
                Transformation(vec3(0.0f, 1.9f, -1.9f), quat::null(), vec3(1.2f, 0.6f, 1.0f))));
    standardCamera(s);
}

inline void normalmap(Setup& s)
{
    /* normals around +z in tangent space: (0.5, 0.5, 1) +- a little */
    auto img = pinArray<float>(8, 8, 3);
    for (unsigned int y = 0; y < 8; y++) {
        for (unsigned int x = 0; x < 8; x++) {
            img[y * 8 + x][0] = 0.5f + 0.3f * (texel01(x, y, 0) - 0.5f);
            img[y * 8 + x][1] = 0.5f + 0.3f * (texel01(x, y, 1) - 0.5f);
            img[y * 8 + x][2] = 0.9f;
        }
    }
    Texture* normals = s.scene.take(createTextureImage(img, LinearizeSRGB_Off));
    Material* floor = s.scene.take(new MaterialGGX(vec3(0.8f), vec2(0.25f, 0.25f)));
    floor->normalTex = normals;
    room(s, floor);
    ceilingLight(s);
    Material* bumpy = s.scene.take(new MaterialLambertian(vec3(0.7f, 0.5f, 0.3f)));
    bumpy->normalTex = normals;
    cube(s, bumpy, vec3(-0.8f, 0.5f, 0.2f), 0.5f);
    Material* shiny = s.scene.take(new MaterialModPhong(vec3(0.3f), vec3(0.6f), 50.0f));
    shiny->normalTex = normals;
    s.scene.take(new MeshInstance(s.scene.take(generateSphere(Transformation(), 12, 6)), shiny, Transformation(vec3(0.9f, 0.5f, 0.5f), quat::null(), vec3(0.5f))));
    standardCamera(s);
}

/* ---- environment maps: no walls, the sky lights the scene ---- */

inline void skyStage(Setup& s)
{
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), s.scene.take(new MaterialLambertian(vec3(0.7f))),
                Transformation(vec3(0.0f), faceUp(), vec3(3.0f, 3.0f, 1.0f))));
    cube(s, s.scene.take(new MaterialGGX(vec3(0.9f, 0.7f, 0.4f), vec2(0.1f, 0.2f))), vec3(-0.9f, 0.5f, 0.2f), 0.5f);
    s.scene.take(new Sphere(vec3(0.9f, 0.5f, 0.4f), 0.5f, s.scene.take(new MaterialMirror(vec3(0.9f)))));
    standardCamera(s);
}

inline Texture* skyTexture(Setup& s)
{
    /* a dim sky with a few bright texels, so that the importance tables are far from uniform */
    auto img = pinArray<float>(16, 8, 3);
    for (unsigned int y = 0; y < 8; y++) {
        for (unsigned int x = 0; x < 16; x++) {
            const bool sun = (x == 11 && y == 5) || (x == 3 && y == 6) || (x == 7 && y == 2);
            for (unsigned int c = 0; c < 3; c++)
                img[y * 16 + x][c] = (sun ? 20.0f : 0.2f) + 0.6f * texel01(x, y, c);
        }
    }
    return s.scene.take(createTextureImage(img, LinearizeSRGB_Off));
}

inline void envEquirect(Setup& s, EnvironmentMapEquiRect::Compatibility compat, int N)
{
    skyStage(s);
    EnvironmentMap* env = s.scene.take(new EnvironmentMapEquiRect(skyTexture(s), compat));
    if (N > 0)
        env->initializeImportanceSampling(N);
}
inline void envMitsuba16(Setup& s) { envEquirect(s, EnvironmentMapEquiRect::CompatibilityMitsuba, 16); }
inline void envSurround12(Setup& s) { envEquirect(s, EnvironmentMapEquiRect::CompatibilitySurroundVideo, 12); }
inline void envMitsubaPlain(Setup& s) { envEquirect(s, EnvironmentMapEquiRect::CompatibilityMitsuba, 0); }

inline void envCube(Setup& s)
{
    skyStage(s);
    Texture* side[6];
    side[0] = s.scene.take(new TextureChecker(vec3(1.5f, 0.3f, 0.2f), vec3(0.3f), 3, 3));
    side[1] = s.scene.take(new TextureChecker(vec3(0.2f, 1.4f, 0.3f), vec3(0.4f), 2, 4));
    side[2] = s.scene.take(new TextureConstant(vec4(2.5f, 2.5f, 2.8f, 2.6f)));
    side[3] = s.scene.take(new TextureConstant(vec4(0.1f, 0.1f, 0.1f, 0.1f)));
    side[4] = imageTexture<float>(s, 4, 4, 3, 1.5f, 0.2f, LinearizeSRGB_Off);
    side[5] = s.scene.take(new TextureChecker(vec3(0.3f, 0.4f, 1.6f), vec3(0.5f), 5, 2));
    s.scene.take(new EnvironmentMapCube(side[0], side[1], side[2], side[3], side[4], side[5]));
}

/* ---- spheres and hot spots ---- */

inline void spheres(Setup& s)
{
    room(s);
    s.scene.take(new Sphere(vec3(0.2f, 2.2f, 0.4f), 0.3f, s.scene.take(new LightDiffuse(vec3(12.0f, 11.0f, 9.0f)))), HotSpot);
    s.scene.take(new Sphere(vec3(-1.0f, 0.5f, 0.3f), 0.5f, s.scene.take(new MaterialLambertian(vec3(0.7f, 0.3f, 0.3f)))));
    s.scene.take(new Sphere(vec3(0.3f, 0.35f, 1.0f), 0.35f, s.scene.take(new MaterialGlass(vec3(0.1f, 0.3f, 0.2f), 1.5f))));
    s.scene.take(new Sphere(vec3(1.4f, 0.5f, -0.4f), 0.5f, s.scene.take(new MaterialGGX(vec3(0.8f), vec2(0.2f, 0.1f)))));
    /* no turned sphere: the reference's sphere tangent does not follow the turn, and every material builds its tangent space
     * from it (an assertion of the reference's stops such a scene) */
    Texture* checker = s.scene.take(new TextureChecker(vec3(0.8f, 0.8f, 0.2f), vec3(0.2f, 0.2f, 0.7f), 8, 4));
    s.scene.take(new Sphere(vec3(0.0f, 1.5f, -1.0f), 0.4f, s.scene.take(new MaterialLambertian(vec3(1.0f), checker))));
    standardCamera(s);
}

inline void hotspots(Setup& s)
{
    room(s);
    ceilingLight(s, vec3(6.0f, 5.0f, 4.0f), 0.7f, vec3(-1.0f, 2.8f, 0.5f));
    ceilingLight(s, vec3(20.0f, 24.0f, 30.0f), 0.12f, vec3(1.3f, 2.5f, -0.2f));
    Material* glow = s.scene.take(new LightDiffuse(vec3(4.0f, 1.0f, 0.5f)));
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), glow,
                Transformation(vec3(2.45f, 0.8f, 0.5f), toQuat(radians(-90.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.5f, 0.2f, 1.0f))), HotSpot);
    s.scene.take(new Sphere(vec3(0.0f, 0.25f, 1.2f), 0.25f, s.scene.take(new LightDiffuse(vec3(2.0f, 3.0f, 2.0f)))), HotSpot);
    cube(s, s.scene.take(new MaterialGGX(vec3(0.8f), vec2(0.15f, 0.15f))), vec3(-0.9f, 0.5f, 0.0f), 0.5f);
    standardCamera(s);
}

/* ---- measured BRDFs ---- */

inline void rglScene(Setup& s, const char* file)
{
    room(s);
    ceilingLight(s);
    Material* m = s.scene.take(new MaterialRGL(s.goldenDir + "/" + file));
    cube(s, m, vec3(-0.9f, 0.5f, 0.2f), 0.5f);
    s.scene.take(new Sphere(vec3(0.9f, 0.5f, 0.5f), 0.5f, m));
    standardCamera(s);
}
inline void rglIso(Setup& s) { rglScene(s, "synthetic_iso.bsdf"); }
inline void rglAniso(Setup& s) { rglScene(s, "synthetic_aniso.bsdf"); }

/* ---- motion ---- */

inline void animation(Setup& s)
{
    room(s);
    ceilingLight(s);
    AnimationKeyframes* slide = new AnimationKeyframes();
    slide->addKeyframe(0.0f, Transformation(vec3(-1.4f, 0.5f, 0.2f), quat::null(), vec3(0.5f)));
    slide->addKeyframe(0.5f, Transformation(vec3(-0.6f, 0.6f, 0.2f), toQuat(radians(40.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.5f)));
    slide->addKeyframe(1.0f, Transformation(vec3(0.0f, 0.5f, 0.6f), toQuat(radians(90.0f), vec3(0.0f, 1.0f, 0.2f)), vec3(0.4f)));
    const int slideIndex = s.scene.take(slide);
    s.scene.take(new MeshInstance(s.scene.take(generateCube()), s.scene.take(new MaterialLambertian(vec3(0.3f, 0.4f, 0.8f))), slideIndex));
    const int rollIndex = s.scene.take(new AnimationKeyframes(
                0.0f, Transformation(vec3(0.6f, 0.35f, 0.8f), quat::null(), vec3(0.35f)),
                1.0f, Transformation(vec3(1.6f, 0.45f, 0.2f), quat::null(), vec3(0.45f))));
    Texture* checker = s.scene.take(new TextureChecker(vec3(0.9f, 0.8f, 0.5f), vec3(0.2f, 0.3f, 0.3f), 6, 3));
    s.scene.take(new Sphere(s.scene.take(new MaterialLambertian(vec3(1.0f), checker)), rollIndex));
    /* the camera takes ownership of its key frames */
    const Animation* travel = new AnimationKeyframes(
            0.0f, Transformation::fromLookAt(vec3(-0.4f, 1.3f, 4.2f), vec3(0.0f, 0.9f, 0.0f)),
            1.0f, Transformation::fromLookAt(vec3(0.5f, 1.5f, 4.0f), vec3(0.1f, 0.8f, 0.0f)));
    s.camera.reset(new Camera(Optics(Projection(radians(50.0f), s.aspect())), travel));
}

/* ---- the camera ---- */

inline void thinlens(Setup& s)
{
    lambertian(s);
    const Optics o(Projection(radians(50.0f), s.aspect()), LensDistortion(), LensDepthOfField(0.25f, 4.0f));
    standardCamera(s, &o);
}

inline void distortion(Setup& s)
{
    lambertian(s);
    const Optics o(Projection(radians(50.0f), s.aspect()), LensDistortion(-0.18f, 0.05f, 0.01f, 0.004f, -0.003f));
    standardCamera(s, &o);
}

inline void distortionRadial(Setup& s)
{
    lambertian(s);
    const Optics o(Projection(radians(50.0f), s.aspect()), LensDistortion(0.12f, -0.03f, 0.002f, 0.001f));
    standardCamera(s, &o);
}

/* ---- the sensor's gates and the integrator's parameters, all on the GGX room ---- */

inline void gatePathLen(Setup& s)
{
    ggx(s);
    s.minPathLen = 6.0f;
    s.maxPathLen = 9.5f;
}
inline void gateDistToLight(Setup& s)
{
    ggx(s);
    s.minDistToLight = 1.5f;
    s.maxDistToLight = 3.4f;
}
/* a path of one component sees only the environment (the reference ends a path at its last component before it adds what
 * the surface emits), so these cases stand under a sky that fills most of the frame, with a lamp besides */
inline void glowRoom(Setup& s, unsigned int maxPathComponents)
{
    s.scene.take(new MeshInstance(s.scene.take(generateQuad()), s.scene.take(new MaterialLambertian(vec3(0.7f))),
                Transformation(vec3(0.0f), faceUp(), vec3(1.6f, 1.6f, 1.0f))));
    ceilingLight(s, vec3(9.0f), 0.3f, vec3(0.0f, 2.6f, 0.3f));
    cube(s, s.scene.take(new MaterialGGX(vec3(0.9f, 0.6f, 0.3f), vec2(0.05f, 0.35f))), vec3(-0.7f, 0.4f, 0.2f), 0.4f);
    cube(s, s.scene.take(new MaterialLambertian(vec3(0.7f, 0.75f, 0.9f))), vec3(0.7f, 0.3f, 0.6f), 0.3f, -20.0f);
    s.scene.take(new EnvironmentMapEquiRect(skyTexture(s)));
    standardCamera(s);
    s.params.maxPathComponents = maxPathComponents;
}
inline void maxPath1(Setup& s) { glowRoom(s, 1); }
inline void maxPath2(Setup& s) { glowRoom(s, 2); }
inline void maxPath4(Setup& s) { glowRoom(s, 4); }
inline void maxPathDefault(Setup& s) { glowRoom(s, Parameters().maxPathComponents); }
inline void rouletteOff(Setup& s) { ggx(s); s.params.rrThreshold = 0.0f; s.params.maxPathComponents = 12; }
inline void pixelCentres(Setup& s) { ggx(s); s.params.randomizeRayOverPixel = false; }

/* ---- a Cornell box whose lamp lies in the ceiling plane: its light rays graze the ceiling and meet the walls' shared
 * edges and corners; boxes stand on the floor so that edges are shared there too ---- */

inline void cornell(Setup& s)
{
    Scene& sc = s.scene;
    Material* white = sc.take(new MaterialLambertian(vec3(0.73f)));
    Material* red = sc.take(new MaterialLambertian(vec3(0.65f, 0.05f, 0.05f)));
    Material* green = sc.take(new MaterialLambertian(vec3(0.12f, 0.45f, 0.15f)));
    const quat turnLeft = toQuat(radians(90.0f), vec3(0.0f, 1.0f, 0.0f)), turnRight = toQuat(radians(-90.0f), vec3(0.0f, 1.0f, 0.0f));
    sc.take(new MeshInstance(sc.take(generateQuad(Transformation(), 3)), white, Transformation(vec3(0.0f, -1.0f, 0.0f), faceUp())));
    sc.take(new MeshInstance(sc.take(generateQuad(Transformation(), 2)), white, Transformation(vec3(0.0f, 1.0f, 0.0f), faceDown())));
    sc.take(new MeshInstance(sc.take(generateQuad(Transformation(), 2)), white, Transformation(vec3(0.0f, 0.0f, -1.0f))));
    sc.take(new MeshInstance(sc.take(generateQuad()), red, Transformation(vec3(-1.0f, 0.0f, 0.0f), turnLeft)));
    sc.take(new MeshInstance(sc.take(generateQuad()), green, Transformation(vec3(1.0f, 0.0f, 0.0f), turnRight)));
    /* the lamp in the ceiling plane itself (y = 1), pointing down */
    sc.take(new MeshInstance(sc.take(generateQuad()), sc.take(new LightDiffuse(vec3(15.0f, 13.0f, 9.0f))),
                Transformation(vec3(0.0f, 1.0f, 0.0f), faceDown(), vec3(0.25f))), HotSpot);
    sc.take(new MeshInstance(sc.take(generateCube()), white,
                Transformation(vec3(-0.35f, -0.4f, -0.3f), toQuat(radians(18.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f, 0.6f, 0.3f))));
    sc.take(new MeshInstance(sc.take(generateCube()), sc.take(new MaterialGGX(vec3(0.8f), vec2(0.2f, 0.2f))),
                Transformation(vec3(0.4f, -0.7f, 0.3f), toQuat(radians(-17.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.3f))));
    s.camera.reset(new Camera(Optics(Projection(radians(40.0f), s.aspect())), Transformation::fromLookAt(vec3(0.0f, 0.0f, 3.7f), vec3(0.0f))));
}

/* ---- time of flight: the lamp at the camera, a diffuse light besides, the scene moves during the exposure ---- */

inline void tof(Setup& s)
{
    Scene& sc = s.scene;
    /* a wall, a panel that slides in front of it during the exposure, an octahedron */
    sc.take(new MeshInstance(sc.take(generateQuad()), sc.take(new MaterialLambertian(vec4(0.85f, 0.8f, 0.75f, 0.8f))),
                Transformation(vec3(0.0f, 0.2f, -2.6f), toQuat(radians(12.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(4.0f, 3.0f, 1.0f))));
    const int slide = sc.take(new AnimationKeyframes(
                0.0f, Transformation(vec3(-1.1f, 0.3f, -1.7f), toQuat(radians(-25.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.4f)),
                1.0f, Transformation(vec3(0.9f, 0.5f, -1.3f), toQuat(radians(15.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.4f))));
    sc.take(new MeshInstance(sc.take(generateQuad()), sc.take(new MaterialModPhong(vec4(0.55f), vec4(0.35f), 60.0f)), slide));
    sc.take(new MeshInstance(sc.take(generateOctahedron()), sc.take(new MaterialLambertian(vec4(0.4f, 0.5f, 0.6f, 0.65f))),
                Transformation(vec3(0.35f, -0.45f, -1.2f), toQuat(radians(33.0f), vec3(0.3f, 1.0f, 0.0f)), vec3(0.4f))));
    /* the modulated lamp just above the camera, looking where it looks; its back side is black */
    Material* front = sc.take(new LightTof(2.75f, radians(110.0f)));
    Material* lamp = sc.take(new MaterialTwoSided(front, sc.take(new MaterialLambertian(vec4(0.0f)))));
    sc.take(new MeshInstance(sc.take(generateQuad()), lamp,
                Transformation(vec3(0.0f, 0.09f, 0.0f), toQuat(radians(180.0f), vec3(0.0f, 1.0f, 0.0f)), vec3(0.07f, 0.04f, 1.0f))), HotSpot);
    /* background light that is not modulated */
    sc.take(new MeshInstance(sc.take(generateQuad()), sc.take(new LightDiffuse(vec4(0.6f, 0.5f, 0.4f, 0.35f))),
                Transformation(vec3(1.7f, 1.4f, -0.6f), toQuat(radians(125.0f), vec3(1.0f, 0.4f, 0.0f)), vec3(0.35f))), HotSpot);
    s.params.maxPathComponents = 4;
    s.camera.reset(new Camera(Optics(Projection(radians(62.0f), s.aspect()))));
}

/* ---- one scene that holds one material of every kind, for the vectors of Material::scatter, scatterToDirection and
 * emitted: `list` receives them in the order in which the scene took them, which is their Scene::materialIndex() ---- */

inline void materialsForProbe(Setup& s, std::vector<const Material*>& list)
{
    Scene& sc = s.scene;
    Texture* checker = sc.take(new TextureChecker(vec3(0.9f, 0.5f, 0.2f), vec3(0.1f, 0.3f, 0.6f), 6, 6));
    Texture* rough = sc.take(new TextureChecker(vec3(0.05f, 0.3f, 0.0f), vec3(0.4f, 0.1f, 0.0f), 5, 5));
    Texture* image = imageTexture<uint8_t>(s, 7, 5, 3, 255.0f, 0.0f);
    auto take = [&](Material* m) {
        list.push_back(sc.take(m));
        return m;
    };
    take(new MaterialLambertian(vec3(0.3f, 0.4f, 0.8f)));
    take(new MaterialLambertian(vec4(0.9f, 0.8f, 0.7f, 0.6f), image));
    take(new LightDiffuse(vec3(9.0f, 8.0f, 7.0f), checker));
    take(new LightSpot(radians(30.0f), vec3(14.0f, 12.0f, 9.0f)));
    take(new LightSpot(radians(70.0f), vec3(14.0f, 12.0f, 9.0f), checker));
    take(new LightSpot(radians(360.0f), vec3(1.0f, 2.0f, 3.0f)));
    take(new MaterialMirror(vec3(0.95f, 0.9f, 0.8f), checker));
    take(new MaterialGlass(vec3(0.0f), 1.5f));
    take(new MaterialGlass(vec3(0.9f, 0.2f, 0.4f), vec3(1.45f, 1.5f, 1.58f)));
    take(new MaterialModPhong(vec3(0.5f), checker, vec3(0.3f), nullptr, 60.0f));
    take(new MaterialModPhong(vec3(0.3f, 0.5f, 0.2f), vec3(0.5f), 120.0f, 0.55f));
    take(new MaterialGGX(vec3(0.9f, 0.6f, 0.3f), vec2(0.05f, 0.35f)));
    take(new MaterialGGX(vec3(0.8f, 0.8f, 0.75f), vec2(0.2f, 0.2f), checker, rough));
    Material* front = take(new MaterialModPhong(vec3(0.5f, 0.3f, 0.2f), vec3(0.4f), 80.0f));
    Material* back = take(new MaterialGGX(vec3(0.3f, 0.6f, 0.8f), vec2(0.15f, 0.25f)));
    take(new MaterialTwoSided(front, back));
    Material* lamp = take(new LightSpot(radians(50.0f), vec3(5.0f, 6.0f, 7.0f), checker));
    Material* dark = take(new MaterialLambertian(vec3(0.0f)));
    take(new MaterialTwoSided(lamp, dark));
    take(new MaterialTwoSided(dark, lamp));
    take(new MaterialRGL(s.goldenDir + "/synthetic_iso.bsdf"));
    take(new MaterialRGL(s.goldenDir + "/synthetic_aniso.bsdf"));
    take(new LightTof(2.5f, radians(100.0f)));
    take(new LightTof(1.5f, radians(140.0f), checker));
    /* every material on a quad of its own, so that the flattened scene carries it */
    for (size_t i = 0; i < list.size(); i++)
        sc.take(new MeshInstance(sc.take(generateQuad()), list[i], Transformation(vec3(2.5f * i, 0.0f, 0.0f))));
    standardCamera(s);
}

/* which cases also give vectors of the reference's classes: hits of its tree and triangles, its hot spots, its
 * environment map (one with importance sampling) */
struct Probe
{
    const char* caseName;
    const char* kind; /* "hits", "hotspots" or "envmap" */
};

inline const std::vector<Probe>& probes()
{
    static const std::vector<Probe> table = {
        { "cornell", "hits" }, { "textures", "hits" },
        { "hotspots", "hotspots" }, { "spot_70", "hotspots" }, { "spheres", "hotspots" },
        { "env_mitsuba_16", "envmap" }, { "env_surround_12", "envmap" },
    };
    return table;
}

/* ---- the table ---- */

inline const std::vector<Case>& cases()
{
    static const std::vector<Case> table = {
        { "lambertian", lambertian, 32, 24, 2, 0.0f, 0.0f, false, "lambertian light_diffuse", "" },
        { "ggx", ggx, 32, 24, 2, 0.0f, 0.0f, false, "ggx checker", "" },
        { "glass", glass, 32, 24, 2, 0.0f, 0.0f, false, "glass", "" },
        { "mirror", mirror, 32, 24, 2, 0.0f, 0.0f, false, "mirror", "" },
        { "modphong", modphong, 32, 24, 2, 0.0f, 0.0f, false, "modphong checker opacity", "" },
        { "twosided", twosided, 32, 24, 2, 0.0f, 0.0f, false, "twosided modphong ggx", "" },
        { "spot_none", spotNone, 32, 24, 3, 0.0f, 0.0f, false, "light_diffuse", "" },
        { "spot_30", spot30, 32, 24, 3, 0.0f, 0.0f, false, "spot", "spot_360 spot_none" },
        { "spot_70", spot70, 32, 24, 3, 0.0f, 0.0f, false, "spot", "spot_360 spot_none spot_30" },
        { "spot_360", spot360, 32, 24, 3, 0.0f, 0.0f, false, "spot", "spot_none" },
        { "spot_70_textured", spot70Textured, 32, 24, 3, 0.0f, 0.0f, false, "spot checker", "spot_360_textured spot_none spot_70" },
        { "spot_360_textured", spot360Textured, 32, 24, 3, 0.0f, 0.0f, false, "spot checker", "spot_none spot_360" },
        { "spot_30_twosided", spot30TwoSided, 32, 24, 3, 0.0f, 0.0f, false, "spot twosided", "spot_360_twosided spot_none" },
        { "spot_360_twosided", spot360TwoSided, 32, 24, 3, 0.0f, 0.0f, false, "spot twosided", "spot_none" },
        { "textures", textures, 32, 24, 2, 0.0f, 0.0f, false, "checker transformer image_u8 image_u16 image_f32", "" },
        { "normalmap", normalmap, 32, 24, 2, 0.0f, 0.0f, false, "normalmap image_f32", "" },
        { "env_mitsuba_16", envMitsuba16, 32, 24, 3, 0.0f, 0.0f, false, "envmap_equirect importance sphere", "env_surround_12" },
        { "env_surround_12", envSurround12, 32, 24, 3, 0.0f, 0.0f, false, "envmap_equirect importance sphere", "" },
        { "env_mitsuba_plain", envMitsubaPlain, 32, 24, 2, 0.0f, 0.0f, false, "envmap_equirect sphere", "env_mitsuba_16" },
        { "env_cube", envCube, 32, 24, 2, 0.0f, 0.0f, false, "envmap_cube sphere", "" },
        { "spheres", spheres, 32, 24, 2, 0.0f, 0.0f, false, "sphere sphere_hotspot glass ggx", "" },
        { "hotspots", hotspots, 32, 24, 2, 0.0f, 0.0f, false, "hotspots sphere_hotspot", "" },
        { "rgl_iso", rglIso, 32, 24, 2, 0.0f, 0.0f, false, "rgl", "" },
        { "rgl_aniso", rglAniso, 32, 24, 2, 0.0f, 0.0f, false, "rgl", "rgl_iso" },
        { "animation", animation, 32, 24, 3, 0.2f, 0.7f, false, "animation camera_animation sphere", "" },
        { "thinlens", thinlens, 32, 24, 2, 0.0f, 0.0f, false, "thinlens", "lambertian" },
        { "distortion", distortion, 32, 24, 2, 0.0f, 0.0f, false, "distortion", "lambertian" },
        { "distortion_radial_planar", distortionRadial, 32, 24, 2, 0.0f, 0.0f, false, "distortion", "lambertian distortion" },
        { "gate_path_len", gatePathLen, 32, 24, 2, 0.0f, 0.0f, false, "gate", "ggx" },
        { "gate_dist_to_light", gateDistToLight, 32, 24, 2, 0.0f, 0.0f, false, "gate", "ggx gate_path_len" },
        { "max_path_default", maxPathDefault, 32, 24, 2, 0.0f, 0.0f, false, "light_diffuse envmap_equirect", "" },
        { "max_path_1", maxPath1, 32, 24, 2, 0.0f, 0.0f, false, "max_path_components", "max_path_default" },
        { "max_path_2", maxPath2, 32, 24, 2, 0.0f, 0.0f, false, "max_path_components", "max_path_default max_path_1" },
        { "max_path_4", maxPath4, 32, 24, 2, 0.0f, 0.0f, false, "max_path_components", "max_path_default max_path_2" },
        { "roulette_off", rouletteOff, 32, 24, 2, 0.0f, 0.0f, false, "roulette_off", "ggx" },
        { "pixel_centres", pixelCentres, 32, 24, 2, 0.0f, 0.0f, false, "pixel_centres", "ggx" },
        { "cornell", cornell, 32, 32, 3, 0.0f, 0.0f, false, "cornell shared_edges", "" },
        { "tof", tof, 32, 24, 2, 0.3f, 0.5f, true, "tof light_tof light_diffuse animation", "" },
    };
    return table;
}

inline const Case* findCase(const std::string& name)
{
    for (const Case& c : cases())
        if (name == c.name)
            return &c;
    return nullptr;
}

/* a case ready to be rendered: built, with its tree bounded for the exposure interval */
inline void setUp(const Case& c, Setup& s, const std::string& goldenDir)
{
    s.width = c.width;
    s.height = c.height;
    s.goldenDir = goldenDir;
    c.build(s);
    s.scene.updateBVH(c.t0, c.t1);
}

}
