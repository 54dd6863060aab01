/*
 * wpt_capi_scene.hip -- of include/wurblpt_hip.h: wpt_scene_upload, _free and _check, what an uploaded scene reports
 * (wpt_scene_folded_links, wpt_scene_bypassed_nodes, the test hook wpt_scene_get_envmap_tables) and the plans of a description
 * (wpt_fold_plan, wpt_bypass_plan).  What an uploaded scene looks like -- validation, the stackless node form and its storage
 * order, the wide form, the triangles' order, the texel and measured-BRDF pools, the environment's tables -- is decided by the
 * pure host functions of wpt_scene_layout.h; wpt_scene_upload copies what they return and runs the three kernels that finish a
 * scene on the device.
 */
#include <cstring>
#include <memory>

#include "wpt_capi_common.h"
#include "wpt_scene_layout.h"
#include "wpt_leaf_words.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

namespace {

/* per-bin importance of the environment map (envmap.hpp:128-140) */
__global__ void wpt_env_importance_kernel(SceneView sv, int N, float* importance)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * N)
        return;
    int x = i % N, y = i / N;
    f2 uv;
    uv.y = ((float)y + 0.5f) / (float)N;
    uv.x = ((float)x + 0.5f) / (float)N;
    f4 L = envL(sv, envInvM(uv));
    importance[i] = L.x + L.y + L.z + L.w;
}

/* per triangle hot spot: what its pdf needs of the corners alone (wpt_blocks.h hotSpotFace; the corners are the world-space
 * positions the walk tests, tri_geom) */
__global__ void wpt_hotspot_face_kernel(SceneView sv, float4* face)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sv.hotspotCount)
        return;
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sv.hotspots[i].kind != WPT_HOTSPOT_SPHERE) {
        const uint32_t p = sv.hotspots[i].prim;
        const float4 g0 = sv.triGeom[3 * p], g1 = sv.triGeom[3 * p + 1], g2 = sv.triGeom[3 * p + 2];
        f = wptk::hotSpotFace(mk3(g0.x, g0.y, g0.z), mk3(g1.x, g1.y, g1.z), mk3(g2.x, g2.y, g2.z));
    }
    face[i] = f;
}

/* decodes one image texture into the RGBA float4 pool (see imageTexelDecode) */
__global__ void wpt_expand_texels_kernel(const uint8_t* pool, const wpt_texture t, float4* out)
{
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= size_t(t.width) * t.height)
        return;
    const f4 v = imageTexelDecode(pool, t, i % t.width, i / t.width);
    out[i] = make_float4(v.x, v.y, v.z, v.w);
}

template<typename T> wpt_status uploadArray(wpt_scene* s, const T* src, size_t count, const T** dst)
{
    *dst = nullptr;
    size_t bytes = count * sizeof(T);
    void* p = nullptr;
    WPT_TRY(hipStatus("hipMalloc", hipMalloc(&p, bytes > 0 ? bytes : 16), true));
    s->allocations.push_back(p);
    if (bytes > 0)
        HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return WPT_OK;
}

wpt_status uploadQuads(wpt_scene* s, const std::vector<wptl::Quad>& quads, const float4** dst)
{
    static_assert(sizeof(wptl::Quad) == sizeof(float4), "the layout's quadwords are the device's");
    return uploadArray(s, reinterpret_cast<const float4*>(quads.data()), quads.size(), dst);
}

wpt_status layoutStatus(const wptl::Status& st)
{
    return st.code == WPT_OK ? WPT_OK : fail(st.code, st.message);
}

/* what wpt_scene_upload owns until its last line, and its temporary device buffers: freed on every way out */
struct SceneFree {
    void operator()(wpt_scene* s) const { wpt_scene_free(s); }
};
struct DeviceFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
using DeviceTemp = std::unique_ptr<void, DeviceFree>;

wpt_status deviceTemp(size_t bytes, const char* what, DeviceTemp* mem)
{
    void* p = nullptr;
    WPT_TRY(hipStatus(what, hipMalloc(&p, bytes > 0 ? bytes : 16), true));
    mem->reset(p);
    return WPT_OK;
}

/* device memory that lives as long as the scene */
wpt_status sceneAlloc(wpt_scene* s, size_t bytes, const char* what, void** p)
{
    WPT_TRY(hipStatus(what, hipMalloc(p, bytes > 0 ? bytes : 16), true));
    s->allocations.push_back(*p);
    return WPT_OK;
}

/* the pool of decoded texels that devTex indexes (wptl::texelOffsets), filled from the caller's raw pool by one launch per image */
wpt_status decodeTexels(wpt_scene* s, const wpt_scene_desc* desc, const std::vector<wpt_texture>& devTex, size_t texelCount)
{
    void* pool = nullptr;
    WPT_TRY(sceneAlloc(s, texelCount * sizeof(float4), "hipMalloc for the decoded texel pool", &pool));
    s->view.texels4 = static_cast<const float4*>(pool);
    if (texelCount == 0)
        return WPT_OK;
    DeviceTemp raw;
    WPT_TRY(deviceTemp(desc->texel_bytes, "texel decode", &raw));
    WPT_TRY(hipStatus("texel decode", hipMemcpy(raw.get(), desc->texels, desc->texel_bytes, hipMemcpyHostToDevice), true));
    for (uint32_t i = 0; i < desc->texture_count; i++) {
        const wpt_texture& t = desc->textures[i];
        if (t.type != WPT_TEX_IMAGE)
            continue;
        const size_t n = size_t(t.width) * t.height;
        hipLaunchKernelGGL(wpt_expand_texels_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, 0,
                static_cast<const uint8_t*>(raw.get()), t, static_cast<float4*>(pool) + devTex[i].texel_offset);
        WPT_TRY(hipStatus("texel decode", hipGetLastError(), true));
    }
    return hipStatus("texel decode", hipDeviceSynchronize(), true);
}

/* SceneView::hotspotFace from the view's hot spots and triangles as uploaded */
wpt_status hotspotFaces(wpt_scene* s)
{
    void* face = nullptr;
    WPT_TRY(sceneAlloc(s, size_t(s->view.hotspotCount) * sizeof(float4), "hot spot faces", &face));
    hipLaunchKernelGGL(wpt_hotspot_face_kernel, dim3((s->view.hotspotCount + 255) / 256), dim3(256), 0, 0, s->view, static_cast<float4*>(face));
    WPT_TRY(hipStatus("hot spot faces", hipDeviceSynchronize(), true));
    s->view.hotspotFace = static_cast<const float4*>(face);
    return WPT_OK;
}

/* per-bin importance of the environment (envmap.hpp:128-140) from the device's own L() over the view as it is */
wpt_status envImportance(const SceneView& view, int N, std::vector<float>* importance)
{
    const size_t bins = size_t(N) * N;
    DeviceTemp dImp;
    WPT_TRY(deviceTemp(bins * sizeof(float), "hipMalloc for the importance map", &dImp));
    hipLaunchKernelGGL(wpt_env_importance_kernel, dim3((bins + 255) / 256), dim3(256), 0, 0, view, N, static_cast<float*>(dImp.get()));
    importance->resize(bins);
    return hipStatus("importance map", hipMemcpy(importance->data(), dImp.get(), bins * sizeof(float), hipMemcpyDeviceToHost), true);
}

uint32_t sceneFeatures(const wpt_scene_desc* d)
{
    uint32_t f = 0;
    for (uint32_t i = 0; i < d->material_count; i++) {
        const wpt_material& m = d->materials[i];
        if (m.type == WPT_MAT_MODPHONG)
            f |= FEAT_MODPHONG;
        if (m.type == WPT_MAT_TWOSIDED)
            f |= FEAT_TWOSIDED;
        if (m.type == WPT_MAT_GGX)
            f |= FEAT_GGX;
        if (m.type == WPT_MAT_GLASS || m.type == WPT_MAT_MIRROR)
            f |= FEAT_GLASS;
        if (m.type == WPT_MAT_LIGHT_SPOT)
            f |= FEAT_SPOT;
        bool tex = m.normal_tex >= 0;
        if (m.type != WPT_MAT_TWOSIDED)
            for (int k = 0; k < 5; k++)
                tex = tex || m.tex[k] >= 0;
        if (tex)
            f |= FEAT_TEXTURES;
    }
    if (d->envmap.type != WPT_ENV_NONE)
        f |= FEAT_ENVMAP | FEAT_TEXTURES;
    if (d->sphere_count > 0)
        f |= FEAT_SPHERES;
    for (uint32_t i = 0; i < d->material_count; i++)
        if (d->materials[i].type == WPT_MAT_RGL)
            f |= FEAT_RGL;
    for (uint32_t i = 0; i < d->instance_count; i++)
        if (d->instances[i].animation >= 0)
            f |= FEAT_ANIM;
    for (uint32_t i = 0; i < d->sphere_count; i++)
        if (d->spheres[i].animation >= 0)
            f |= FEAT_ANIM;
    return f;
}

/* wptl::validate, its message kept for wpt_last_error */
wpt_status validate(const wpt_scene_desc* d)
{
    return layoutStatus(wptl::validate(d));
}

} /* namespace */

extern "C" {

/* Lay out, copy, release: one array at a time (wpt_scene_layout.h says what each looks like; DESIGN.md section 3 has the table),
 * then the three kernels that finish the scene on the device, each reading the view as it is at that moment. */
wpt_status wpt_scene_upload(const wpt_scene_desc* desc, wpt_scene** out_scene)
{
    if (!out_scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "out_scene is NULL");
    *out_scene = nullptr;
    WPT_TRY(validate(desc));
    if (wpt_device_count() <= 0)
        return fail(WPT_ERR_NO_DEVICE, "no HIP device is available; the path tracer has no CPU fallback");
    /* the process's hooks, read once: what the scene looks like on the device is a function of the description and these two */
    const uint32_t walk = settings.walk, topNodes = settings.topNodes;
    std::unique_ptr<wpt_scene, SceneFree> owner(new wpt_scene);
    wpt_scene* s = owner.get();
    SceneView& view = s->view;
    HIP_TRY(hipGetDevice(&s->device));
    s->features = sceneFeatures(desc);
    s->nodeCount = desc->node_count;
    s->triCount = desc->tri_count;
    memset(&view, 0, sizeof(view));
    const std::vector<uint32_t> triNew = wptl::triangleOrder(desc, (walk & WPT_WALK_TRIANGLES_AS_GIVEN) != 0);
    const bool fitsLds = size_t(desc->node_count) * 32 + size_t(desc->tri_count) * 48 <= LDS_SCENE_MAX_BYTES;
    std::vector<uint32_t> ldsNodes; /* the device nodes of a tree that fits LDS, kept for its link words below */
    {
        wptl::DeviceNodes nodes;
        WPT_TRY(layoutStatus(wptl::deviceNodes(desc, triNew, topNodes, &nodes)));
        view.nodeCount = desc->node_count;
        view.boxesMayBeNan = nodes.boxesMayBeNan;
        WPT_TRY(uploadQuads(s, nodes.quads, &view.nodes));
        s->foldedLinks = 0;
        if (fitsLds) { /* the trees that are walked from LDS */
            s->foldedLinks = wptl::countFoldedLinks(reinterpret_cast<const uint32_t*>(nodes.quads.data()), desc->node_count, nullptr);
            ldsNodes.resize(size_t(desc->node_count) * 8);
            memcpy(ldsNodes.data(), nodes.quads.data(), ldsNodes.size() * 4);
        }
    }
    if (walk & WPT_WALK_WIDE) {
        const std::vector<wptl::Quad> wide = wptl::wideNodes(desc, triNew);
        if (!wide.empty()) /* a tree without a wide form is walked as it is */
            WPT_TRY(uploadQuads(s, wide, &view.wideNodes));
    }
    {
        const std::vector<wpt_tri_geom> g = wptl::permuted(desc->tri_geom, triNew);
        WPT_TRY(uploadArray(s, reinterpret_cast<const float4*>(g.data()), size_t(desc->tri_count) * 3, &view.triGeom));
        if (fitsLds) {
            /* the link words of the tree's copy in LDS, computed once per scene: the exact ones, plain and folded, and the
             * ones that go round the nodes the plan leaves out (wpt_bypass.h) */
            const wptb::Plan plan = wptb::plan(ldsNodes.data(), desc->node_count, g.data(), desc->tri_count, settings.bypassMode);
            std::vector<uint32_t> words(plan.plain);
            words.insert(words.end(), plan.folded.begin(), plan.folded.end());
            words.insert(words.end(), plan.bypass.begin(), plan.bypass.end());
            s->leafOneToOne = true;
            for (const std::vector<uint32_t>* links : { &plan.plain, &plan.folded, &plan.bypass }) {
                const wptw::LeafWords leaf = wptw::leafWords(links->data(), desc->node_count, desc->tri_count);
                if (leaf.verdict == wptw::TOO_LARGE)
                    return fail(WPT_ERR_UNSUPPORTED, "a tree that fits LDS has indices beyond its leaf words");
                s->leafOneToOne = s->leafOneToOne && leaf.verdict == wptw::ONE_TO_ONE;
                words.insert(words.end(), leaf.words.begin(), leaf.words.end());
            }
            const uint32_t* onDevice = nullptr;
            WPT_TRY(uploadArray(s, words.data(), words.size(), &onDevice));
            s->ldsLinks = const_cast<uint32_t*>(onDevice);
            s->bypassedNodes = plan.outCount;
            /* the ordered box copies, for a tree that has them */
            std::vector<wptl::Quad> ordered;
            if (wptl::orderedBoxCopies(ldsNodes.data(), desc->node_count, &ordered))
                WPT_TRY(uploadQuads(s, ordered, &s->orderedNodes));
        }
    }
    {
        const std::vector<wpt_tri_attr> a = wptl::permuted(desc->tri_attr, triNew);
        WPT_TRY(uploadArray(s, reinterpret_cast<const float4*>(a.data()), size_t(desc->tri_count) * 6, &view.triAttr));
    }
    WPT_TRY(uploadArray(s, desc->instances, desc->instance_count, &view.instances));
    s->normalsNamed = wptl::normalsNamed(desc);
    WPT_TRY(uploadArray(s, desc->materials, desc->material_count, &view.materials));
    view.materialCount = desc->material_count;
    {
        size_t texelCount = 0;
        const std::vector<wpt_texture> devTex = wptl::texelOffsets(desc, &texelCount);
        WPT_TRY(uploadArray(s, devTex.data(), devTex.size(), &view.textures));
        WPT_TRY(decodeTexels(s, desc, devTex, texelCount));
    }
    {
        const std::vector<wpt_hotspot> h = wptl::remappedHotspots(desc, triNew);
        WPT_TRY(uploadArray(s, h.data(), h.size(), &view.hotspots));
    }
    WPT_TRY(uploadArray(s, desc->spheres, desc->sphere_count, &view.spheres));
    WPT_TRY(uploadArray(s, desc->rgl_brdfs, desc->rgl_count, &view.rglBrdfs));
    {
        const wptl::RglPool rgl = wptl::rglPool(desc);
        WPT_TRY(uploadArray(s, rgl.pool.data(), rgl.pool.size(), &view.rglData));
        WPT_TRY(uploadArray(s, rgl.rgbl.data(), rgl.rgbl.size(), &view.rglRgbl));
    }
    WPT_TRY(uploadArray(s, desc->animations, desc->animation_count, &view.animations));
    WPT_TRY(uploadArray(s, desc->keyframes, desc->keyframe_count, &view.keyframes));
    s->animationCount = desc->animation_count;
    view.sphereCount = desc->sphere_count;
    for (int k = 0; k < 6; k++)
        view.envCube[k] = desc->envmap.cube_tex[k];
    {
        hipDeviceProp_t prop;
        s->cuCount = hipGetDeviceProperties(&prop, s->device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    view.triCount = desc->tri_count;
    view.hotspotCount = desc->hotspot_count;
    view.invHotspotCount = desc->hotspot_count ? 1.0f / float(desc->hotspot_count) : 0.0f;
    if (desc->hotspot_count > 0)
        WPT_TRY(hotspotFaces(s));
    view.envType = desc->envmap.type;
    view.envCompat = desc->envmap.compat;
    view.envTex = desc->envmap.tex;
    view.envN = 0;
    view.envLog2N = -1;
    if (desc->envmap.type != WPT_ENV_NONE && desc->envmap.N > 0) {
        const int N = desc->envmap.N;
        const size_t bins = size_t(N) * N;
        if (desc->envmap.M && desc->envmap.Ms && desc->envmap.Mcs) {
            s->envM.assign(desc->envmap.M, desc->envmap.M + bins);
            s->envMs.assign(desc->envmap.Ms, desc->envmap.Ms + bins);
            s->envMcs.assign(desc->envmap.Mcs, desc->envmap.Mcs + bins);
        } else {
            /* the per-bin importance comes from the device's own L(); the tables from it on the host */
            std::vector<float> importance;
            WPT_TRY(envImportance(view, N, &importance));
            wptl::EnvTables t = wptl::envTablesFromImportance(importance.data(), bins);
            s->envM.swap(t.M);
            s->envMs.swap(t.Ms);
            s->envMcs.swap(t.Mcs);
        }
        WPT_TRY(uploadArray(s, s->envM.data(), bins, &view.envM));
        WPT_TRY(uploadArray(s, s->envMs.data(), bins, &view.envMs));
        WPT_TRY(uploadArray(s, s->envMcs.data(), bins, &view.envMcs));
        const std::vector<int32_t> lut = wptl::envStartTable(s->envMcs.data(), bins);
        if (!lut.empty()) { /* a caller's own table that is not monotone gets the plain bisection */
            WPT_TRY(uploadArray(s, lut.data(), lut.size(), &view.envLut));
            view.envLutSize = wptl::ENV_LUT_SIZE;
        }
        view.envN = N;
        view.envLog2N = wptl::envLog2(N);
    }
    *out_scene = owner.release();
    return WPT_OK;
}

void wpt_scene_free(wpt_scene* scene)
{
    if (!scene)
        return;
    for (void* p : scene->allocations)
        (void)hipFree(p);
    delete scene;
}

/* copies the importance tables of an uploaded scene back (tests compare them with the oracle's) */
wpt_status wpt_scene_get_envmap_tables(const wpt_scene* scene, float* M, int32_t* Ms, float* Mcs)
{
    if (!scene || scene->view.envN <= 0)
        return fail(WPT_ERR_INVALID_ARGUMENT, "scene has no importance tables");
    size_t bins = scene->envM.size();
    memcpy(M, scene->envM.data(), bins * sizeof(float));
    memcpy(Ms, scene->envMs.data(), bins * sizeof(int32_t));
    memcpy(Mcs, scene->envMcs.data(), bins * sizeof(float));
    return WPT_OK;
}

/* Waits for the device and reports an error of any launch since the last call (a fault inside a kernel surfaces
 * here).  The kernels themselves have no bounded waits that could run out: every loop ends with its work. */
wpt_status wpt_scene_check(wpt_scene* scene)
{
    if (!scene)
        return fail(WPT_ERR_INVALID_ARGUMENT, "scene is NULL");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipGetLastError());
    return WPT_OK;
}

wpt_status wpt_scene_folded_links(const wpt_scene* scene, uint32_t* folded)
{
    if (!scene || !folded)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *folded = scene->foldedLinks;
    return WPT_OK;
}

wpt_status wpt_fold_plan(const wpt_scene_desc* desc, uint32_t* folded, uint32_t* lds_words)
{
    if (!folded)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(validate(desc));
    /* the device nodes of wpt_scene_upload with nothing in front (depth-first: the storage order of every tree that fits LDS)
     * and the triangles as given */
    wptl::DeviceNodes nodes;
    WPT_TRY(layoutStatus(wptl::deviceNodes(desc, wptl::triangleOrder(desc, true), 0, &nodes)));
    *folded = wptl::countFoldedLinks(reinterpret_cast<const uint32_t*>(nodes.quads.data()), desc->node_count, lds_words);
    return WPT_OK;
}

wpt_status wpt_scene_bypassed_nodes(const wpt_scene* scene, uint32_t* count)
{
    if (!scene || !count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = scene->bypassedNodes;
    return WPT_OK;
}

wpt_status wpt_bypass_plan(const wpt_scene_desc* desc, uint32_t* count, uint32_t* words)
{
    if (!count)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    WPT_TRY(validate(desc));
    /* as wpt_fold_plan: the description's own depth-first order and triangle indices */
    wptl::DeviceNodes nodes;
    WPT_TRY(layoutStatus(wptl::deviceNodes(desc, wptl::triangleOrder(desc, true), 0, &nodes)));
    const uint32_t* n = reinterpret_cast<const uint32_t*>(nodes.quads.data());
    *count = 0;
    std::vector<uint32_t> links;
    if (size_t(desc->node_count) * 32 + size_t(desc->tri_count) * 48 <= LDS_SCENE_MAX_BYTES) {
        const wptb::Plan plan = wptb::plan(n, desc->node_count, desc->tri_geom, desc->tri_count, settings.bypassMode);
        *count = plan.outCount;
        links = plan.bypass;
    } else { /* a tree that is not walked from LDS has no plan: the fold's links */
        links = wptb::linkWords(n, desc->node_count, true, nullptr);
    }
    if (words) {
        memcpy(words, links.data(), 2 * size_t(desc->node_count) * 4);
        words[2 * size_t(desc->node_count)] = links[2 * size_t(desc->node_count) + 2]; /* the node a ray starts at */
    }
    return WPT_OK;
}

} /* extern "C" */
