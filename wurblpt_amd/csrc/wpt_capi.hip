/*
 * wpt_capi.hip -- of include/wurblpt_hip.h: devices, names and build info; what the last launch ran (wpt_last_*, wpt_kernel_name,
 * wpt_kernel_form); every wpt_set_* but the despeckle form's; the planners that need no device (wpt_kernel_choice,
 * wpt_kernel_table_entry, wpt_launch_plan, wpt_slices_plan, wpt_split_plan, wpt_device_lanes).  The state that the units share
 * (wpt_capi_common.h) is defined here, and the constants that the host-only headers restate are held to the kernels'.  This unit
 * has no kernel and launches none.
 */
#include <atomic>
#include <cstring>

#include "wpt_capi_common.h"
#include "wpt_scene_layout.h"
#include "wpt_leaf_words.h"
#include "wpt_streams.h"

using namespace wptd;
using namespace wptk;
using namespace wptc;

namespace {

thread_local std::string g_error; /* wpt_last_error */

/* what the process's most recent render call ran: kernel launches it took for its pixels (wpt_last_render_passes) and which
 * kernel family (wpt_kernel_name).  Process-wide, so that a caller whose worker threads render (MPICoordinator, bench.py's
 * block queue) reads on its main thread what the workers ran. */
std::atomic<uint32_t> g_lastPasses{1};
std::atomic<const char*> g_kernelName{nullptr};
std::atomic<const char*> g_kernelForm{""}; /* wpt_kernel_form */

/* the pair of counters the most recent render call's kernel adds to (wpt_last_slice_stats), or NULL if it was not sliced */
std::atomic<unsigned long long*> g_lastSliceStats{nullptr};

/* lanes per workgroup of the most recent render call's path-tracing kernel, bit 31: its boxes were ordered (wpt_kernel_workgroup) */
std::atomic<uint32_t> g_lastWorkgroup{uint32_t(WG)};
/* WPT_HIT_DATA_* of the parts the most recent render call's kernel kept in LDS (wpt_kernel_hit_data) */
std::atomic<uint32_t> g_lastHitData{0};
/* 1: that kernel read the material records by LDS address (wpt_kernel_materials_in_lds) */
std::atomic<uint32_t> g_lastMaterialsInLds{0};
/* 1: that kernel read the launch's constants from the launch record in LDS (wpt_kernel_launch_record) */
std::atomic<uint32_t> g_lastLaunchRecord{0};
static_assert(WPT_HIT_DATA_RECORDS == wptk::HIT_DATA_RECORDS && WPT_HIT_DATA_HOTSPOTS == wptk::HIT_DATA_HOTSPOTS && WPT_HIT_DATA_NORMALS == wptk::HIT_DATA_NORMALS,
        "wpt_lds_places.h restates the header's names of the parts");

static_assert(wptk::PLAN_WG == uint32_t(WG) && wptk::PLAN_SLICE_SLOT_MAX == wptk::SLICE_SLOT_MASK && wptk::SLICE_UNITS_TARGET <= wptk::SLICE_UNITS_MAX
        && wptk::PLAN_FRAME == wptk::SENSOR_FRAME && wptk::PLAN_VIEWS == wptk::SENSOR_VIEWS && wptk::PLAN_ADAPTIVE == wptk::SENSOR_ADAPTIVE
        && wptk::PLAN_SENSORS == wptk::SENSOR_COUNT, "wpt_launch_plan.h restates the kernels' constants and the sensors");
static_assert(wptl::NODE_CHILD == NODE_CHILD && wptl::NODE_INDEX_MASK == NODE_INDEX_MASK && wptl::PRIM_SPHERE == PRIM_SPHERE && wptl::WIDE_STACK == WIDE_STACK
        && wptl::WIDE_NONE == WIDE_NONE && wptl::LDS_SCENE_MAX_BYTES == LDS_SCENE_MAX_BYTES && wptl::ORDERED_COPIES == wptk::ORDERED_COPIES,
        "wpt_scene_layout.h restates the kernels' node words and limits");
static_assert(wptw::LEAF_NODE_SHIFT == wptk::LEAF_NODE_SHIFT && wptw::LEAF_NODE_MAX == wptk::LEAF_NODE_MAX && wptw::LEAF_CORNER_MASK == wptk::LEAF_CORNER_MASK
        && LDS_SCENE_MAX_BYTES / 32 <= wptw::LEAF_NODE_MAX && LDS_SCENE_MAX_BYTES / 16 <= wptw::LEAF_CORNER_MASK,
        "wpt_leaf_words.h restates the rotated kernels' leaf word, which has room for every tree that fits LDS");

} /* namespace */

namespace wptc {

Settings settings;

wpt_status fail(wpt_status s, const std::string& msg)
{
    g_error = msg;
    return s;
}

/* What the process's most recent render call ran, all of it at once: every path that renders stores it here and nowhere else
 * (the wavefront form and the stages of a session too).  sliceStats: the counters a sliced launch adds to, else NULL. */
void recordLaunch(const char* name, const char* form, uint32_t passes, unsigned long long* sliceStats)
{
    g_kernelName.store(name, std::memory_order_relaxed);
    g_kernelForm.store(form, std::memory_order_relaxed);
    g_lastPasses.store(passes, std::memory_order_relaxed);
    g_lastSliceStats.store(sliceStats, std::memory_order_relaxed);
    g_lastWorkgroup.store(uint32_t(WG), std::memory_order_relaxed);
    g_lastHitData.store(0, std::memory_order_relaxed);
    g_lastMaterialsInLds.store(0, std::memory_order_relaxed);
    g_lastLaunchRecord.store(0, std::memory_order_relaxed);
}

/* ... and, behind recordLaunch, the workgroup of a launch that was not one of WG lanes with the plain node array, and the parts
 * of a hit's data it kept in LDS, the material records by LDS address among them or not, and the launch record with them or not */
void recordWorkgroup(uint32_t lanes, bool orderedBoxes, uint32_t hitDataParts, bool materialsByLdsAddress, bool launchRecord)
{
    g_lastMaterialsInLds.store(materialsByLdsAddress ? 1u : 0u, std::memory_order_relaxed);
    g_lastLaunchRecord.store(launchRecord ? 1u : 0u, std::memory_order_relaxed);
    g_lastWorkgroup.store(lanes | (orderedBoxes ? 0x80000000u : 0u), std::memory_order_relaxed);
    g_lastHitData.store(hitDataParts, std::memory_order_relaxed);
}

/* wpt_kernel_form of a launch: "rotated corners" for that form of the kernel with the scene in LDS -- with ", leaf links from
 * the nodes" where the scene's tree is not one leaf per triangle and the leaf pass reads the leaf's node (wpt_leaf_words.h) --
 * and ", sliced xU" behind it for a launch that hands its pixels out in U > 1 units */
const char* kernelForm(bool rotated, uint32_t units, bool leafLinksFromNodes)
{
    static const std::vector<std::string> forms = [] {
        std::vector<std::string> f;
        for (int r = 0; r < 3; r++)
            for (uint32_t u = 0; u <= wptk::SLICE_UNITS_MAX; u++)
                f.push_back(std::string(r ? "rotated corners" : "") + (r == 2 ? ", leaf links from the nodes" : "")
                        + (u > 1 ? ", sliced x" + std::to_string(u) : std::string()));
        return f;
    }();
    return forms[(rotated ? (leafLinksFromNodes ? 2 : 1) * (wptk::SLICE_UNITS_MAX + 1) : 0) + (units <= wptk::SLICE_UNITS_MAX ? units : 0)].c_str();
}

/* the kernel table's row for an instantiation; there is no launch without one */
wpt_status lookupKernel(uint32_t features, bool count, bool ldsScene, bool wide, const wptk::KernelEntry** entry)
{
    *entry = wptk::findKernel(features, count, ldsScene, wide);
    if (!*entry)
        return fail(WPT_ERR_UNSUPPORTED, "the library has no kernel wpt_pathtrace<F = " + std::to_string(features) + ", COUNT = " + std::to_string(count)
                + ", LDSSCENE = " + std::to_string(ldsScene) + ", WIDE = " + std::to_string(wide) + ">");
    return WPT_OK;
}

} /* namespace wptc */

extern "C" {

int wpt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        g_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return 0;
    }
    return n;
}

wpt_status wpt_select_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return WPT_OK;
}

wpt_status wpt_current_device(int* device)
{
    if (!device)
        return fail(WPT_ERR_INVALID_ARGUMENT, "device is NULL");
    HIP_TRY(hipGetDevice(device));
    return WPT_OK;
}

const char* wpt_device_name(int device)
{
    thread_local std::string name;
    name.clear();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        name = std::string(prop.name) + " (" + prop.gcnArchName + ", " + std::to_string(prop.multiProcessorCount) + " CUs)";
    return name.c_str();
}

wpt_status wpt_device_lanes(int device, uint32_t* lanes)
{
    if (!lanes)
        return fail(WPT_ERR_INVALID_ARGUMENT, "device lanes: NULL argument");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    *lanes = uint32_t(prop.multiProcessorCount) * 1024u;
    return WPT_OK;
}

const char* wpt_build_info(void)
{
#if defined(__clang_version__)
    return "hipcc / clang " __clang_version__ ", --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt "
           "-fno-gpu-flush-denormals-to-zero";
#else
    return "unknown compiler";
#endif
}

const char* wpt_last_error(void)
{
    return g_error.c_str();
}

const char* wpt_kernel_name(void)
{
    /* the kernel family of the process's most recent render call */
    const char* name = g_kernelName.load(std::memory_order_relaxed);
    return name ? name : "wpt_pathtrace";
}

const char* wpt_kernel_form(void)
{
    return g_kernelForm.load(std::memory_order_relaxed);
}

uint32_t wpt_kernel_workgroup(uint32_t* ordered_boxes)
{
    const uint32_t w = g_lastWorkgroup.load(std::memory_order_relaxed);
    if (ordered_boxes)
        *ordered_boxes = w >> 31;
    return w & 0x7fffffffu;
}

uint32_t wpt_kernel_hit_data(void)
{
    return g_lastHitData.load(std::memory_order_relaxed);
}

uint32_t wpt_kernel_materials_in_lds(void)
{
    return g_lastMaterialsInLds.load(std::memory_order_relaxed);
}

uint32_t wpt_kernel_launch_record(void)
{
    return g_lastLaunchRecord.load(std::memory_order_relaxed);
}

int wpt_material_places(uint32_t node_count, uint32_t tri_count, uint32_t material_count, uint32_t behind_corners, uint32_t instance_count,
        uint32_t hotspot_count, uint32_t* at, uint32_t* quads)
{
    const wptk::MaterialPlaces m = wptk::launchMaterialPlaces(node_count, tri_count, material_count, behind_corners != 0, instance_count, hotspot_count);
    if (at)
        *at = m.at;
    if (quads)
        *quads = m.quads;
    return m.in ? 1 : 0;
}

uint32_t wpt_last_render_passes(void)
{
    return g_lastPasses.load(std::memory_order_relaxed);
}

wpt_status wpt_last_slice_stats(uint64_t* taken, uint64_t* continued)
{
    if (!taken || !continued)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    *taken = 0;
    *continued = 0;
    const unsigned long long* stats = g_lastSliceStats.load(std::memory_order_relaxed);
    if (!stats)
        return WPT_OK;
    unsigned long long host[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, stats, sizeof(host), hipMemcpyDeviceToHost));
    *taken = host[0];
    *continued = host[1];
    return WPT_OK;
}

wpt_status wpt_set_launch_config(uint32_t threads_per_group, uint32_t variant)
{
    if (threads_per_group != 0 && threads_per_group != WG)
        return fail(WPT_ERR_UNSUPPORTED, "this build uses 256 threads per workgroup");
    settings.threadsPerGroup = WG;
    settings.variant = variant & 0xffu;
    settings.leaveEighths = 0;
    settings.heavyMin = 0;
    settings.leafBias = 0;
    if ((variant >> 8) & 0xffu)
        settings.leaveEighths = ((variant >> 8) & 0xffu) - 1; /* byte 1: leave threshold in eighths, plus one */
    if ((variant >> 16) & 0xffu)
        settings.heavyMin = ((variant >> 16) & 0xffu) - 1;     /* byte 2: lanes a long block needs, plus one */
    if ((variant >> 24) & 0xffu)
        settings.leafBias = (variant >> 24) & 0xffu;           /* byte 3: leaf bias */
    return WPT_OK;
}

wpt_status wpt_set_wavefront(uint32_t mode, uint32_t groups, uint32_t chunk, uint32_t flags)
{
    if (mode > 2u)
        return fail(WPT_ERR_INVALID_ARGUMENT, "wavefront mode must be 0, 1 or 2");
    settings.wfMode = mode;
    settings.wfConfig.groups = groups & 0xffu;
    settings.wfConfig.tracePerCu = (groups >> 8) & 0xffu; /* measurements: workgroups of the trace per compute unit */
    settings.wfConfig.shadePerKind = (groups >> 16) & 1u; /* measurements: one shade launch per kind of material */
    settings.wfConfig.chunk = chunk;
    settings.wfConfig.buckets = (flags & 1u) ? 0u : 1u;
    settings.wfConfig.refillIdle = (flags >> 8) & 0x3fu;
    settings.wfConfig.leafBias = 0;
    /* bits 16-31: node steps a ray takes per launch of the trace before it is suspended (0 = default, 0xffff = no limit) */
    settings.wfConfig.stepBudget = (flags >> 16) == 0xffffu ? 0xffffffffu : (flags >> 16);
    /* bits 1-7: nodes in front of the node array that the trace walks from LDS, in units of 128 (0 = default, 0x7f = none) */
    settings.wfConfig.topNodes = ((flags >> 1) & 0x7fu) == 0x7fu ? 0xffffffffu : ((flags >> 1) & 0x7fu) * 128u;
    return WPT_OK;
}

wpt_status wpt_set_top_nodes(uint32_t nodes)
{
    settings.topNodes = nodes & 0x7fffffffu;
    return WPT_OK;
}

wpt_status wpt_set_walk(uint32_t flags)
{
    if (flags & ~(WPT_WALK_WIDE | WPT_WALK_FULL_SHADOW | WPT_WALK_COUNT_PRODUCT | WPT_WALK_TRIANGLES_AS_GIVEN | WPT_WALK_SELECT_CORNERS | WPT_WALK_NO_FOLD | WPT_WALK_NO_BYPASS
            | WPT_WALK_SMALL_WORKGROUPS | WPT_WALK_HIT_DATA_IN_HBM))
        return fail(WPT_ERR_INVALID_ARGUMENT, "unknown walk flag");
    settings.walk = flags;
    return WPT_OK;
}

wpt_status wpt_set_slices(uint32_t n)
{
    if ((n & ~WPT_SLICES_DECLINE_ODD) > wptk::SLICE_UNITS_MAX)
        return fail(WPT_ERR_INVALID_ARGUMENT, "slices: 0 (the library's plan), 1 (never) or 2 .. 15 units, with or without WPT_SLICES_DECLINE_ODD");
    settings.slices = n;
    return WPT_OK;
}

wpt_status wpt_set_bypass(uint32_t mode)
{
    if (mode > wptb::MODE_ALL_ELIGIBLE)
        return fail(WPT_ERR_INVALID_ARGUMENT, "bypass mode: 0 (the cost model's choice) or 1 (every eligible inner node)");
    settings.bypassMode = mode;
    return WPT_OK;
}

/* profiling hook: device buffer of 11 uint64 that counted launches add their wave-scheduler
 * statistics to (rounds, loop iterations and lane counts per state); NULL switches it off */
wpt_status wpt_set_scheduler_stats(unsigned long long* stats_device)
{
    settings.schedStats = stats_device;
    return WPT_OK;
}

wpt_status wpt_slices_plan(uint32_t block_size, uint32_t lanes_at_once, uint32_t samples_sqrt, uint32_t* units, uint32_t* rows)
{
    if (!units || !rows)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    wptk::slicesPlan(block_size, lanes_at_once, samples_sqrt, units, rows);
    return WPT_OK;
}

wpt_status wpt_kernel_choice(uint32_t need, uint32_t sensor, uint32_t count, uint32_t node_count, uint32_t tri_count, uint32_t material_count,
        uint32_t scene_has_wide, uint32_t variant, uint32_t walk, const char** name, const char** form, uint32_t key[4],
        uint64_t* scene_lds_bytes, uint32_t* materials_in_lds)
{
    if (!name || !form || !key || !scene_lds_bytes || !materials_in_lds)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor: 0 frame, 1 transient, 2 views, 3 adaptive, 4 time of flight");
    const wptk::KernelChoice choice = wptk::selectKernel({ need, wptk::Sensor(sensor), count != 0, node_count, tri_count, material_count,
            scene_has_wide != 0, variant, walk });
    const wptk::KernelEntry* kernel = nullptr;
    const wpt_status found = lookupKernel(choice.features, choice.count, choice.ldsScene, choice.wide, &kernel);
    if (found != WPT_OK)
        return found;
    *name = kernel->name;
    *form = kernelForm(choice.rotated);
    key[0] = kernel->features;
    key[1] = kernel->count;
    key[2] = kernel->ldsScene;
    key[3] = kernel->wide;
    *scene_lds_bytes = choice.sceneLdsBytes;
    *materials_in_lds = choice.materialsInLds;
    return WPT_OK;
}

wpt_status wpt_launch_plan(uint32_t sensor, uint32_t count, uint32_t need, uint32_t scene_in_lds, uint32_t block_size, uint32_t samples_sqrt,
        uint32_t cu_count, uint32_t variant, uint32_t wavefront_mode, uint32_t slices, uint32_t plan[WPT_PLAN_WORDS])
{
    if (!plan)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sensor >= wptk::SENSOR_COUNT)
        return fail(WPT_ERR_INVALID_ARGUMENT, "sensor: 0 frame, 1 transient, 2 views, 3 adaptive, 4 time of flight");
    if (wavefront_mode > 2u)
        return fail(WPT_ERR_INVALID_ARGUMENT, "wavefront mode must be 0, 1 or 2");
    const wptk::LaunchPlan p = wptk::planLaunch({ sensor, count != 0, (need & FEAT_RGL) != 0, (need & FEAT_ANIM) != 0, scene_in_lds != 0,
            block_size, samples_sqrt, cu_count, variant, wavefront_mode, slices });
    const uint32_t words[WPT_PLAN_WORDS] = { p.wavefront, p.wavefrontFallBack, p.pooled, p.strategy, p.units, p.rows, p.passes };
    memcpy(plan, words, sizeof(words));
    return WPT_OK;
}

wpt_status wpt_kernel_table_entry(uint32_t index, uint32_t key[4], const char** name)
{
    if (!key || !name)
        return fail(WPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (index >= wptk::KERNEL_TABLE_ROWS)
        return fail(WPT_ERR_INVALID_ARGUMENT, "the kernel table has " + std::to_string(wptk::KERNEL_TABLE_ROWS) + " rows");
    const wptk::KernelEntry& k = wptk::KERNEL_TABLE[index];
    key[0] = k.features;
    key[1] = k.count;
    key[2] = k.ldsScene;
    key[3] = k.wide;
    *name = k.name;
    return WPT_OK;
}

wpt_status wpt_split_plan(uint64_t pixels, uint32_t samples_sqrt, uint32_t lanes, uint32_t* stream_count, uint32_t* stream_samples_sqrt)
{
    if (!stream_count || !stream_samples_sqrt)
        return fail(WPT_ERR_INVALID_ARGUMENT, "split plan: NULL argument");
    if (!wptstr::splitPlan(pixels, samples_sqrt, lanes, stream_count, stream_samples_sqrt))
        return fail(WPT_ERR_INVALID_ARGUMENT, "split plan: pixels, samples_sqrt and lanes must be above 0");
    return WPT_OK;
}

} /* extern "C" */
