/*
 * wurblpt_hip.h -- C ABI of the MI355X (gfx950) path-tracing core.
 *
 * This is the drop-in boundary for the one hot path of WurblPT: the per-pixel
 * Monte Carlo integrator.  The reference has no FFI of its own; everything is
 * inlined from headers into the applications (reference libwurblpt/wurblpt.hpp:279-449).
 * The entry points below are what the reference-side `mcpt()` binds instead of
 * running its OpenMP pixel loop (wurblpt.hpp:335-381):
 *
 *   wpt_scene_upload()   replaces the data that `mcpt` borrows from `Scene`:
 *                        scene.bvh() (bvh.hpp:217-225,277-311), the HitableTriangle objects
 *                        (hitable_triangle.hpp:46-143), Mesh vertex data (mesh.hpp:39-66),
 *                        Material / Texture objects (material*.hpp, texture*.hpp),
 *                        scene.hotSpots() and scene.environmentMap() (scene.hpp:173-191)
 *   wpt_render_block()   replaces one iteration of the block loop: the OpenMP pixel loop,
 *                        Prng(pixel), the sample loop, Camera::getRay, tracePath and
 *                        Sensor::finishPixel (wurblpt.hpp:319-383, sensor_rgb.hpp:63-87)
 *   MPICoordinator::getBlock/submitBlock (mpi.hpp:241-262) stay on the caller's side: blocks are
 *   plain (start, size) arguments (include/wurblpt/mpi.hpp, wurblpt_amd/blocks.py)
 *
 * All structs are plain C PODs; the caller keeps ownership of everything it
 * passes in (the callee copies during wpt_scene_upload).  No C++ types, no
 * exceptions and no torch types cross this boundary.  Functions return an
 * integer status; wpt_last_error() gives a thread-local message.
 *
 * Thread compatibility: a wpt_scene belongs to the device that was current
 * when it was uploaded; concurrent wpt_render_block* calls on one scene are
 * allowed when they use different streams and disjoint pixel ranges.
 */
#ifndef WURBLPT_HIP_H
#define WURBLPT_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WPT_ABI_VERSION 5u

typedef enum {
    WPT_OK = 0,
    WPT_ERR_INVALID_ARGUMENT = 1,
    WPT_ERR_NO_DEVICE = 2,
    WPT_ERR_HIP = 3,
    WPT_ERR_UNSUPPORTED = 4,
    WPT_ERR_OUT_OF_MEMORY = 5
} wpt_status;

/* ---- flattened scene ------------------------------------------------- */

/* One node of the depth-first linearized BVH; 32 bytes like BVHNodeLinear
 * (bvh.hpp:217-225).  Child 1 of an inner node is the next node in the array
 * (bvh.hpp:301), child 2 is `link`.  For a leaf, `link` is the index of the triangle or sphere. */
enum { WPT_NODE_INNER = 0, WPT_NODE_TRIANGLE = 1, WPT_NODE_SPHERE = 2, WPT_NODE_EMPTY = 3 };
typedef struct wpt_bvh_node {
    float lo[3];
    float hi[3];
    uint32_t link;
    uint32_t kind;
} wpt_bvh_node;

/* Triangle flags; mirror the HitableTriangle template arguments (hitable_triangle.hpp:36) */
enum { WPT_TRI_HAVE_TEXCOORDS = 1, WPT_TRI_HAVE_TANGENTS = 2, WPT_TRI_TRANSFORM = 4, WPT_TRI_ANIMATE = 8 };

/* Intersection stream: world-space positions of one triangle (48 bytes).  With
 * WPT_TRI_TRANSFORM the positions are the instance's mat4 applied on the host with
 * the arithmetic of hitable_triangle.hpp:203-206, which is the value hit() recomputes per call.
 * With WPT_TRI_ANIMATE the instance's animation at the ray's time is applied to them in the
 * kernel (hitable_triangle.hpp:209-218). */
typedef struct wpt_tri_geom {
    float v0[3];
    uint32_t instance;
    float v1[3];
    uint32_t material;
    float v2[3];
    uint32_t flags;
} wpt_tri_geom;

/* Shading stream: de-indexed vertex attributes of one triangle (96 bytes), read once per
 * final hit (hitable_triangle.hpp:289-322).  Unused members are zero. */
typedef struct wpt_tri_attr {
    float n0[3], n1[3], n2[3];
    float tc0[2], tc1[2], tc2[2];
    float t0[3], t1[3], t2[3];
} wpt_tri_attr;

/* MeshInstance data needed at hit time (mesh.hpp:159-189): the normal matrix (column major). */
typedef struct wpt_instance {
    float N[9];
    uint32_t material;
    uint32_t flags;
    int32_t animation; /* MeshInstance::animationIndex: index into wpt_scene_desc::animations, -1 = none */
} wpt_instance;

/* Animations (animation_keyframes.hpp): key frames sorted by time; the transformation at a time is the
 * first / last key frame outside their range and mix() of the two neighbours inside (translation and
 * scaling linear, rotation by slerp).  The pool also holds the camera's animation (wpt_camera::animation). */
typedef struct wpt_keyframe {
    float t;
    float translation[3];
    float rotation[4]; /* quaternion x, y, z, w */
    float scaling[3];
} wpt_keyframe;
typedef struct wpt_animation {
    uint32_t first_keyframe;
    uint32_t keyframe_count;
} wpt_animation;

/* A sphere (HitableSphere, hitable_sphere.hpp:32-76): centre = T.translation, radius =
 * max(T.scaling), rotation = T.rotation (turns the normal into texture space). 48 bytes. */
typedef struct wpt_sphere {
    float center[3];
    float radius;
    float rotation[4]; /* quaternion x, y, z, w */
    uint32_t material;
    int32_t animation; /* HitableSphere::_animationIndex: index into wpt_scene_desc::animations, -1 = none */
    uint32_t reserved[2];
} wpt_sphere;

/* A hot spot (scene.hpp:113-125).  WPT_HOTSPOT_TRIANGLE: `prim` is the triangle, plus what
 * HitableTriangle::direction() needs (hitable_triangle.hpp:425-443): untransformed positions
 * and the instance mat4.  WPT_HOTSPOT_SPHERE: `prim` is the sphere; nothing else is used
 * (HitableSphere::pdfValue/direction, hitable_sphere.hpp:149-220, read the sphere record). */
enum { WPT_HOTSPOT_TRIANGLE = 0, WPT_HOTSPOT_SPHERE = 1 };
typedef struct wpt_hotspot {
    uint32_t prim;
    uint32_t transform;
    uint32_t kind;
    int32_t animation; /* of the triangle's instance, -1 = none */
    float p0[3], p1[3], p2[3];
    float M[16];
} wpt_hotspot;

enum {
    WPT_MAT_NONE = 0,          /* base Material: no scattering, no emission (material.hpp:158-185) */
    WPT_MAT_LAMBERTIAN = 1,    /* material_lambertian.hpp */
    WPT_MAT_LIGHT_DIFFUSE = 2, /* light_diffuse.hpp */
    WPT_MAT_MIRROR = 3,        /* material_mirror.hpp */
    WPT_MAT_GGX = 4,           /* material_ggx.hpp */
    WPT_MAT_GLASS = 5,         /* material_glass.hpp */
    WPT_MAT_MODPHONG = 6,      /* material_modphong.hpp */
    WPT_MAT_TWOSIDED = 7,      /* material.hpp:273-334 */
    WPT_MAT_RGL = 8,           /* material_rgl.hpp:46-102, measured BRDF (powitacq_rgb) */
    WPT_MAT_LIGHT_SPOT = 9     /* light_spot.hpp */
};
enum {
    WPT_MATF_HAVE_NIR = 1,
    WPT_MATF_CHROMATIC_DISPERSION = 2,
    WPT_MATF_DIFFUSE_TEX_HAS_ALPHA = 4,
    WPT_MATF_SPECULAR_TEX_HAS_ALPHA = 8,
    /* WPT_MAT_LIGHT_SPOT only: the light is a time-of-flight light (light_tof.hpp).  v[0] = (0, 0, 0, radiance); a texture
     * scales the fourth channel by its red value; what a ToF sensor receives from it is modulated (wpt_render_tof_block) */
    WPT_MATF_TOF_LIGHT = 16
};
/* Tagged material record (128 bytes).  Member use per type:
 *  LAMBERTIAN     v[0]=albedo                      tex[0]=albedo
 *  LIGHT_DIFFUSE  v[0]=emit                        tex[0]=emit
 *  MIRROR         v[0]=color                       tex[0]=color
 *  GGX            v[0]=albedo f[0..1]=roughness    tex[0]=albedo tex[1]=roughness
 *  GLASS          v[0]=absorption v[1]=RI material v[2]=RI surrounding
 *  MODPHONG       v[0]=diffuse v[1]=specular v[2]=transmissive v[3]=emissive
 *                 f[0]=shininess f[1]=opacity f[2]=indexOfRefraction
 *                 tex[0]=diffuse tex[1]=specular tex[2]=shininess tex[3]=opacity tex[4]=emissive
 *  TWOSIDED       tex[0]=front material index, tex[1]=back material index
 *  RGL            tex[0]=index into wpt_scene_desc::rgl_brdfs
 *  LIGHT_SPOT     v[0]=emit (rgb, average) f[0]=cos(openingAngle / 2)   tex[0]=emit
 * Texture indices are -1 when absent. */
typedef struct wpt_material {
    uint32_t type;
    uint32_t flags;
    int32_t normal_tex;
    int32_t tex[5];
    float v[5][4];
    float f[4];
} wpt_material;

/* One interpolant / sample warp of the measured-BRDF model (Marginal2D<Dimension> of
 * powitacq_rgb.inl:183-640): a size_x x size_y grid of bilinear patches per parameter slice.
 * All arrays live in wpt_scene_desc::rgl_data at the given offsets (in floats) and hold what the
 * model's constructor computes (powitacq_rgb.inl:213-310): `data` normalised, and for the warps
 * that are sampled the marginal and conditional CDFs (WPT_RGL_NONE otherwise). */
#define WPT_RGL_NONE 0xffffffffu
typedef struct wpt_rgl_warp {
    uint32_t size_x, size_y;
    uint32_t dims;            /* 0, 2 or 3 parameters */
    uint32_t param_size[3];
    uint32_t param_stride[3];
    uint32_t param_values[3]; /* offsets of the parameter grids */
    uint32_t data, marginal_cdf, conditional_cdf;
    float patch_size[2], inv_patch_size[2];
} wpt_rgl_warp;

/* powitacq_rgb::BRDF::Data (powitacq_rgb.inl:856-864) */
typedef struct wpt_rgl_brdf {
    wpt_rgl_warp ndf, sigma, vndf, luminance, rgb;
    uint32_t isotropic;
    uint32_t jacobian;
} wpt_rgl_brdf;

enum { WPT_TEX_CONSTANT = 0, WPT_TEX_CHECKER = 1, WPT_TEX_IMAGE = 2, WPT_TEX_TRANSFORMER = 3 };
enum { WPT_TEXEL_U8 = 0, WPT_TEXEL_U16 = 1, WPT_TEXEL_F32 = 2 };
/* Texture record (texture.hpp:160-246, texture_image.hpp:39-233).
 *  CONSTANT     a = color
 *  CHECKER      a = color0, b = color1, width = horiz, height = vert
 *  IMAGE        width/height/comps/texel_type/linearize_srgb, texel_offset (bytes into the
 *               texel pool, row 0 = v 0, x fastest, components interleaved),
 *               coord_factor/coord_offset, a = valFactor, b = valOffset
 *  TRANSFORMER  child, coord_factor/coord_offset, a = valFactor, b = valOffset */
typedef struct wpt_texture {
    uint32_t type;
    uint32_t width, height;
    uint32_t comps;
    uint32_t texel_type;
    uint32_t linearize_srgb;
    int32_t child;
    uint32_t reserved;
    uint64_t texel_offset;
    float coord_factor[2];
    float coord_offset[2];
    float a[4];
    float b[4];
} wpt_texture;

enum { WPT_ENV_NONE = 0, WPT_ENV_EQUIRECT = 1, WPT_ENV_CUBE = 2 };
enum { WPT_ENV_COMPAT_MITSUBA = 0, WPT_ENV_COMPAT_SURROUND_VIDEO = 1 };
/* Environment map (envmap.hpp): texture(s) + host-built importance tables (envmap.hpp:121-158).
 * N == 0 means no importance sampling support.  EQUIRECT uses `tex` (envmap.hpp:213-247),
 * CUBE uses `cube_tex` in the order +x -x +y -y +z -z (envmap.hpp:250-285). */
typedef struct wpt_envmap {
    uint32_t type;
    uint32_t compat;
    int32_t tex;
    int32_t N;
    const float* M;
    const int32_t* Ms;
    const float* Mcs;
    int32_t cube_tex[6];
} wpt_envmap;

typedef struct wpt_scene_desc {
    uint32_t abi_version; /* WPT_ABI_VERSION */
    uint32_t node_count;
    uint32_t tri_count;
    uint32_t instance_count;
    uint32_t material_count;
    uint32_t texture_count;
    uint32_t hotspot_count;
    uint32_t sphere_count;
    uint64_t texel_bytes;
    const wpt_bvh_node* nodes;
    const wpt_tri_geom* tri_geom;
    const wpt_tri_attr* tri_attr;
    const wpt_instance* instances;
    const wpt_material* materials;
    const wpt_texture* textures;
    const uint8_t* texels;
    const wpt_hotspot* hotspots;
    wpt_envmap envmap;
    const wpt_sphere* spheres;
    uint32_t rgl_count;      /* measured BRDFs (WPT_MAT_RGL) */
    uint32_t reserved;
    uint64_t rgl_data_count; /* floats in rgl_data */
    const wpt_rgl_brdf* rgl_brdfs;
    const float* rgl_data;
    uint32_t animation_count;
    uint32_t keyframe_count;
    const wpt_animation* animations;
    const wpt_keyframe* keyframes;
} wpt_scene_desc;

/* ---- camera, parameters ---------------------------------------------- */

enum { WPT_SURROUND_OFF = 0, WPT_SURROUND_180 = 1, WPT_SURROUND_360 = 2 };
enum { WPT_DISTORTION_NONE = 0, WPT_DISTORTION_RADIAL_AND_PLANAR = 1, WPT_DISTORTION_RADIAL_ONLY = 2, WPT_DISTORTION_OPENCV = 3 };
/* What Camera::getRay needs for a static pinhole / thin lens camera
 * (camera.hpp:123-185, optics.hpp:37-69,311-334, transformation.hpp:48-83). */
typedef struct wpt_camera {
    float l, r, b, t;        /* Projection frustum at near = 1 */
    float translation[3];
    float rotation[4];       /* quaternion x, y, z, w */
    float scaling[3];
    float lens_radius;
    float focus_dist;
    /* LensDistortion (optics.hpp:112-309) and its per-frame helper (:203-212, from the projection):
     * undistort() maps the distorted image coordinates of a sample to the ones a ray is made from */
    uint32_t distortion_type; /* WPT_DISTORTION_* */
    float k1, k2, k3, p1, p2;
    float b1, b2, b3, b4;     /* RadialOnly: coefficients of the exact inverse (:176-180) */
    float dist_center[2], dist_focal_length[2], dist_inverse_focal_length[2];
    /* Camera::surroundMode and ::stereoscopicDistance (camera.hpp:45-52,128-170): 180 / 360 degree
     * cameras ignore the optics; a stereoscopic camera renders the left view into the upper half */
    uint32_t surround_mode; /* WPT_SURROUND_* */
    float stereoscopic_distance;
    /* Camera::animation: index into the scene's animation pool or -1.  translation / rotation / scaling
     * above hold Camera::at(t0); with t0 != t1 a ray takes the animation at its own time (camera.hpp:175-180). */
    int32_t animation;
} wpt_camera;

/* Parameters (wurblpt.hpp:79-96) plus the SensorRGB gates (sensor_rgb.hpp:41-51). */
typedef struct wpt_params {
    uint32_t max_path_components;
    float rr_threshold;
    uint32_t randomize_ray_over_pixel;
    float min_hit_distance;
    float min_dist_to_light, max_dist_to_light;
    float min_path_len, max_path_len;
    float t0, t1; /* mcpt()'s exposure interval: with t0 != t1 every camera ray draws its time in it (motion blur) */
} wpt_params;

/* Work counters of one render call; the roofline denominator. */
typedef struct wpt_counters {
    uint64_t samples;
    uint64_t rays;          /* BVH::hit calls */
    uint64_t node_visits;   /* nodes fetched in BVH::hit */
    uint64_t leaf_tests;    /* triangle tests in BVH::hit */
    uint64_t pdf_tests;     /* hot-spot pdfValue triangle tests */
    uint64_t scatters;      /* Material::scatter calls */
} wpt_counters;

typedef struct wpt_scene wpt_scene;

/* ---- entry points ---------------------------------------------------- */

/* Number of HIP devices (0 if none); selects the device for this thread. */
int wpt_device_count(void);
wpt_status wpt_select_device(int device);
wpt_status wpt_current_device(int* device); /* the calling thread's HIP device */

/* Copies the flattened scene to the current device. */
wpt_status wpt_scene_upload(const wpt_scene_desc* desc, wpt_scene** out_scene);
void wpt_scene_free(wpt_scene* scene);

/* Renders pixels [block_start, block_start + block_size) of a width x height frame with
 * samples_sqrt^2 samples per pixel, asynchronously on `hip_stream` (NULL = default stream).
 * `frame_device` is a device pointer to the FULL frame, float[height][width][3], row 0 =
 * bottom row (camera.hpp:146-149); only the block's pixels are written.
 * `counters_device` may be NULL; otherwise a device pointer to one wpt_counters that the
 * kernel atomically adds to. */
wpt_status wpt_render_block_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream);

/* One rank's interleaved share of the frame in ONE launch: the frame is cut into bands of `band_rows` rows and this
 * call renders bands first_band, first_band + band_stride, first_band + 2 band_stride, ... (rank r of N: first_band = r,
 * band_stride = N).  Same results as rendering those bands as blocks; a GPU keeps all of the rank's pixels resident
 * without one stream per block.  band_rows a multiple of 8 (and width too) keeps the 8x8 pixel tiles per wave. */
wpt_status wpt_render_bands_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream);

/* Synchronous form for host frames: renders the same bands and writes their pixels into `frame_host`, the FULL frame
 * float[height][width][3] in host memory; the other bands are left as they are (several devices fill one frame). */
wpt_status wpt_render_bands(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host);

/* Synchronous form with MPICoordinator::submitBlock semantics (mpi.hpp:256-262):
 * writes block_size*3 floats for the block's pixels to host memory `block_rgb`. */
wpt_status wpt_render_block(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size, float* block_rgb);

/* ---- rolling shutter ----
 * The frame's rows are exposed one after the other, as a CMOS sensor reads them out: one row every `row_time`, from the top row
 * down (from_top = 1) or from the bottom row up (from_top = 0).  For a frame of `height` rows and the pixels of frame row y
 * (row 0 = bottom, whatever block or band the launch renders):
 *
 *     k = from_top ? height - 1 - y : y        the row's place in the readout
 *     s = (float)k * row_time                  one rounding
 *     a = t0 + s ;  b = t1 + s                 one rounding each
 *
 * and the row is exposed over [a, b] as the plain render exposes the frame over [t0, t1]: row y of the rolling frame is bit for
 * bit row y of wpt_render_block_device with params.t0 = a, params.t1 = b.  The decision is taken per row on a != b: then every
 * camera ray draws its time as a + u * (b - a), and a moving camera is taken at that time.  With a == b (instant rows: t0 == t1,
 * the classic rolling shutter without motion blur) nothing is drawn, the ray's time is a, a camera with animation >= 0 is taken
 * where its animation has it at a, and a camera without one uses its record.  row_time == 0 is the plain render, kernel and
 * all; any other row_time takes the moving-scene kernels, never the wavefront form.
 * Valid: row_time finite and >= 0, from_top 0 or 1, reserved words 0, and the interval of the row read last finite; anything
 * else is refused with WPT_ERR_INVALID_ARGUMENT.  The readout spans [t0, b(k = height - 1)] (wpt_shutter_span): a scene with
 * moving triangles must be bounded for that span, not for [t0, t1].
 * Progressive sessions, the transient / light-group / time-of-flight / adaptive sensors, batches of views and the ground truth
 * take no shutter. */
typedef struct wpt_shutter {
    float row_time;
    uint32_t from_top;
    uint32_t reserved[2]; /* 0 */
} wpt_shutter;

/* Device-free: the interval [*a, *b] of frame row `row` (< height), and the span [*first, *last] of the whole readout, by the
 * rule above.  An invalid shutter is refused with a message, as the render calls refuse it. */
wpt_status wpt_shutter_row_interval(const wpt_shutter* shutter, float t0, float t1, uint32_t height, uint32_t row, float* a, float* b);
wpt_status wpt_shutter_span(const wpt_shutter* shutter, float t0, float t1, uint32_t height, float* first, float* last);

/* wpt_render_block_device, wpt_render_bands_device, wpt_render_bands and wpt_render_block with a shutter (NULL is refused);
 * every other argument means what it means there. */
wpt_status wpt_render_shutter_block_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const wpt_shutter* shutter, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size,
        float* frame_device, wpt_counters* counters_device, void* hip_stream);
wpt_status wpt_render_shutter_bands_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const wpt_shutter* shutter, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_device, wpt_counters* counters_device, void* hip_stream);
wpt_status wpt_render_shutter_bands(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, const wpt_shutter* shutter,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
        float* frame_host);
wpt_status wpt_render_shutter_block(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const wpt_shutter* shutter, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        uint32_t block_start, uint32_t block_size, float* block_rgb);

/* ---- transient film (light-in-flight rendering) ----
 * One launch renders the frame and bin_count planes: plane k holds the light whose optical path length lies in
 * [edges[k], edges[k + 1]), per channel, behind the distance gate of `params` (its path-length gate applies to the frame
 * only).  Plane k is bit-identical to the frame rendered with min_path_len = edges[k] and
 * max_path_len = nextafterf(edges[k + 1], -INFINITY) (FLT_MAX for an infinite last edge); light outside
 * [edges[0], edges[bin_count]) goes to no plane.  `edges_host`: bin_count + 1 increasing floats in host memory, all finite
 * except that the last may be +INFINITY; 1 <= bin_count <= WPT_TRANSIENT_MAX_BINS.  A bad edge set is refused with
 * WPT_ERR_INVALID_ARGUMENT before anything else is looked at.  The planes cost bin_count * width * height * 12 bytes. */
#define WPT_TRANSIENT_MAX_BINS 4096u

/* Asynchronous on `hip_stream`.  `frame_device` (may be NULL): the FULL frame as for wpt_render_block_device;
 * `bins_device`: float[bin_count][height][width][3] in device memory, full frames, row 0 = bottom.  Only the block's
 * pixels are written, in the frame and in every plane. */
wpt_status wpt_render_transient_block_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const float* edges_host, uint32_t bin_count,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, float* bins_device, void* hip_stream);

/* Synchronous form with MPICoordinator::submitBlock semantics: `block_rgb` (may be NULL) receives block_size*3 floats,
 * `block_bins` bin_count*block_size*3 floats (plane k's block_size*3 floats after plane k-1's), both in host memory. */
wpt_status wpt_render_transient_block(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const float* edges_host, uint32_t bin_count,
        uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* block_rgb, float* block_bins);

/* ---- light groups: a frame per group of emitters from one render pass ----
 * One launch renders the frame and group_count planes: plane g holds every contribution whose emitter is in group g.  The
 * emitter of a contribution is the resolved material of the hit whose emission is evaluated (inside a two-sided material: the
 * child), for the path's own hits and for the light ray's hit alike; for the environment's contributions it is `env_group`.
 * Nothing that steers a path reads an emitted radiance, so plane g is bit-identical to the frame of a plain render of the same
 * description with the emission of every material outside group g set to 0 (v[0] of LIGHT_DIFFUSE / LIGHT_SPOT; v[3] of
 * MODPHONG with tex[4] = -1, since an emission texture stands in that factor's place), wherever the full frame is finite.  Both gates of `params` apply to the planes as they do to the frame, and the
 * frame of the launch is the frame of wpt_render_block_device.  The launch is a launch of the transient film's kernels
 * (wpt_kernel_name() reports them) that chooses a contribution's plane by its emitter instead of by its path length.
 * `group_of_material`: one byte per material record of the scene, in host memory, each a group below group_count or
 * WPT_LIGHT_GROUP_NONE (the emitter's light reaches the frame only); `material_count` must be the scene's; `env_group`: a group or
 * WPT_LIGHT_GROUP_NONE; 1 <= group_count <= WPT_LIGHT_GROUPS_MAX.  A bad table is refused with WPT_ERR_INVALID_ARGUMENT before
 * anything else is looked at.  The planes cost group_count * width * height * 12 bytes. */
#define WPT_LIGHT_GROUPS_MAX 255u
#define WPT_LIGHT_GROUP_NONE 0xffu

/* Asynchronous on `hip_stream`.  `frame_device` (may be NULL): the FULL frame as for wpt_render_block_device;
 * `planes_device`: float[group_count][height][width][3] in device memory, full frames, row 0 = bottom.  Only the block's
 * pixels are written, in the frame and in every plane. */
wpt_status wpt_render_light_groups_block_device(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count,
        uint32_t env_group, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* frame_device, float* planes_device, void* hip_stream);

/* Synchronous form with MPICoordinator::submitBlock semantics: `block_rgb` (may be NULL) receives block_size*3 floats,
 * `block_planes` group_count*block_size*3 floats (plane g's block_size*3 floats after plane g-1's), both in host memory. */
wpt_status wpt_render_light_groups_block(wpt_scene* scene, const wpt_camera* camera,
        const wpt_params* params, const uint8_t* group_of_material, uint32_t material_count, uint32_t group_count,
        uint32_t env_group, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* block_rgb, float* block_planes);

/* Planes mixed into one frame with an RGB weight per plane (a group's intensity and colour, chosen after the render):
 *   out[p][c] = (((0 + w[0][c] * P0[p][c]) + w[1][c] * P1[p][c]) + ...)   in float, every operation rounded on its own.
 * `planes_device`: plane k's `pixels` RGB triples start `stride` floats after plane k-1's (light-group planes or the transient
 * film's bins); `weights_host`: plane_count * 3 floats in host memory; 1 <= plane_count <= WPT_TRANSIENT_MAX_BINS.
 * Asynchronous on `hip_stream`.  The host form computes the same bits on the CPU and needs no device. */
wpt_status wpt_postproc_mix_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_device, void* hip_stream);
wpt_status wpt_postproc_mix_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        const float* weights_host, float* out_host);

/* ---- time-of-flight sensor (amplitude-modulated continuous wave; sensor_tof_amcw.hpp) ----
 * One launch renders phase_count phase images of one exposure interval.  Plane j holds, per pixel, the energies (a_j, b_j, total)
 * that the sensor's two taps and their sum collect with the phase offset tau[j]: every contribution adds
 *   energy = radiance.w * 1000 * pixel_area * 0.5 * exposure_time  to total (radiance.w: the near infrared channel),
 *   0.5 * energy * (1 + t) to a and 0.5 * energy * (1 - t) to b, with
 *   t = contrast * cos(tau[j] + 2 pi * opl.w * frac_modfreq_c)  for light emitted by a ToF light (WPT_MATF_TOF_LIGHT), else 0
 * (sensor_tof_amcw.hpp:227-252 in float, operation for operation), and the plane is the sum times 1 / samples.  A pixel's paths
 * depend on its index only, so plane j is bit-identical to a launch with phase_count = 1 and tau[0] = tau[j], and `total` is the
 * same in every plane.  The sensor has no gates: `params` must carry the default ones (min_dist_to_light = min_path_len = 0,
 * max_dist_to_light = max_path_len = FLT_MAX).  Single kernel, one device.  Refused with WPT_ERR_INVALID_ARGUMENT before a
 * device is needed: NULL pointers, a phase count outside 1 .. WPT_TOF_MAX_PHASES, sensor values that are NaN or infinite, a
 * contrast outside [0, 1], gates that are not the defaults. */
#define WPT_TOF_MAX_PHASES 8u
typedef struct wpt_tof_sensor {
    float pixel_area;     /* [um^2] */
    float exposure_time;  /* of one phase image [us] */
    float contrast;       /* achievable pixel contrast in [0, 1] */
    float frac_modfreq_c; /* (float)(modulation frequency [Hz] / speed of light [m/s]), the division made in double */
    uint32_t phase_count;
    float tau[WPT_TOF_MAX_PHASES]; /* phase offsets; SensorTofAmcw: tau[j] = j * (2.0f * pi) / phase_count */
} wpt_tof_sensor;

/* Asynchronous on `hip_stream`.  `planes_device`: float[phase_count][height][width][3] in device memory, full frames,
 * row 0 = bottom.  Only the block's pixels are written, in every plane. */
wpt_status wpt_render_tof_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const wpt_tof_sensor* sensor, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* planes_device, void* hip_stream);

/* Synchronous form with MPICoordinator::submitBlock semantics: `block_planes` receives phase_count * block_size * 3 floats
 * in host memory (plane j's block_size * 3 floats after plane j-1's). */
wpt_status wpt_render_tof_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        const wpt_tof_sensor* sensor, uint32_t width, uint32_t height, uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size,
        float* block_planes);

/* One contribution on the CPU, by the code the kernels run (wpt_tof.h): adds to acc = (a, b, total) of phase `phase`. */
wpt_status wpt_tof_accumulate_host(const wpt_tof_sensor* sensor, uint32_t phase, float radiance_w, float opl_w, int is_tof_light,
        float acc[3]);

/* ---- a batch of views ----
 * One launch renders view_count frames of one scene: frame v from cameras_host[v], with one parameter set, one frame size and one
 * sample count for all.  The cameras may differ in anything (pose, frustum, thin lens, distortion, surround or stereo mode,
 * animation).  Frame v is bit-identical to the plain render of camera v (wpt_render_block_device over the whole frame): a
 * pixel's generator is seeded from its index in its own frame.  The batch is rendered by the single kernel (never in the
 * wavefront form) for the union of the scene's and all cameras' features.  Refused with WPT_ERR_INVALID_ARGUMENT before a
 * device is needed: view_count == 0, NULL cameras or frames, a camera animation index below -1, and
 * view_count * width * height > WPT_VIEWS_MAX_PIXELS; then, with the scene at hand, an animation index outside its array. */
#define WPT_VIEWS_MAX_PIXELS 0x7fffffffu

/* Asynchronous on `hip_stream`.  `frames_device`: float[view_count][height][width][3] in device memory, full frames, row 0 =
 * bottom.  `counters_device` (may be NULL): ONE wpt_counters that receives the sum over all views (added to). */
wpt_status wpt_render_views_device(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        float* frames_device, wpt_counters* counters_device, void* hip_stream);

/* Synchronous form: `frames_host` as above, in host memory. */
wpt_status wpt_render_views(wpt_scene* scene, const wpt_camera* cameras_host, uint32_t view_count,
        const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host);

/* ---- sample streams ----
 * Stream k of a width x height frame is the render in which pixel p's generator is seeded from the index p + k * width * height
 * instead of p: seed = (uint64)p + (uint64)k * (uint64)(width * height) + 42, then splitmix64 twice as ever.  Everything else is
 * the plain render, the strata and the factors 1 / n and 1 / n^2 included.  Stream 0 is the plain render bit for bit; the streams
 * of one frame never share a seed index, and consecutive indices are what neighbouring pixels have.  Streams are a second,
 * independent sample sequence for a pixel: renders of different streams can be averaged, within one launch (so that a small
 * frame fills the device) or across calls and devices.
 *
 * A batch of views with a stream per view: view v is rendered from cameras_host[v] as stream streams_host[v].  streams_host:
 * view_count numbers in host memory, or NULL for all 0, which is wpt_render_views[_device]; those are calls of these.  Frames,
 * counters, kernels and refusals are those of a batch of views. */
wpt_status wpt_render_view_streams_device(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host,
        uint32_t view_count, const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt,
        float* frames_device, wpt_counters* counters_device, void* hip_stream);
wpt_status wpt_render_view_streams(wpt_scene* scene, const wpt_camera* cameras_host, const uint32_t* streams_host,
        uint32_t view_count, const wpt_params* params, uint32_t width, uint32_t height, uint32_t samples_sqrt, float* frames_host);

/* A split render: one camera in stream_count streams first_stream .. first_stream + stream_count - 1 of stream_samples_sqrt^2
 * samples each, in ONE launch of the batch-of-views kernels into stream-ordered scratch (stream_count * width * height * 12
 * bytes, allocated and freed in stream order), then one reduce (wpt_postproc_mean_planes over the scratch):
 *   frame   = ((f_first + f_first+1) + ...) * (1 / (float)stream_count)         a float sum in stream order,
 *   moments = ((f_first^2 + f_first+1^2) + ...) * (1 / (float)stream_count)     every operation rounded on its own.
 * frame: float[height][width][3], row 0 = bottom; moments (may be NULL): the same shape, the stream moment film.  With
 * N = stream_count it is what the variance formula of the adaptive moment film expects, (moments - frame^2) * N / (N - 1) / N,
 * and estimates the variance of the pixel's mean from stream_count independent stream means -- unbiased whatever the strata
 * within a stream, unlike the per-sample moment film.  For stream_count a perfect square, wpt_postproc_denoise takes frame and
 * moments as they are with samples_sqrt = sqrt(stream_count).  With stream_count == 1 and first_stream == 0 the frame is the
 * plain render's bits.  counters_device (may be NULL): the sum over all streams, added to.
 * Refused with WPT_ERR_INVALID_ARGUMENT before a device is needed: stream_count == 0, a NULL frame,
 * stream_count * width * height > WPT_VIEWS_MAX_PIXELS and first_stream + stream_count beyond 2^32.
 * Progressive sessions, adaptive maps, the transient, light-group and time-of-flight films and the wavefront form take no streams. */
wpt_status wpt_render_split_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_device, float* moments_device,
        wpt_counters* counters_device, void* hip_stream);
/* Synchronous form: frame_host and moments_host (may be NULL) in host memory. */
wpt_status wpt_render_split(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t stream_samples_sqrt, uint32_t first_stream, uint32_t stream_count, float* frame_host, float* moments_host);

/* The reduce on its own: the mean of plane_count planes of `pixels` RGB triples that start `stride` floats apart, in plane order
 * as above, and with moment_out (may be NULL) the mean of their squares.  Asynchronous on `hip_stream`, one lane per value, no
 * scratch.  Refused: NULL planes or mean_out, plane_count == 0, pixels == 0, planes that overlap (stride < pixels * 3 with more
 * than one plane).  The host form computes the same bits on the CPU and needs no device; where a result is NaN both are NaN, but
 * the NaN's sign and payload may differ (inf - inf is a negative NaN on x86, a positive one on the GPU).  The same holds for the
 * merge below. */
wpt_status wpt_postproc_mean_planes(const float* planes_device, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_device, float* moment_out_device, void* hip_stream);
wpt_status wpt_postproc_mean_planes_host(const float* planes_host, uint32_t plane_count, uint64_t stride, uint64_t pixels,
        float* mean_out_host, float* moment_out_host);

/* Two results of disjoint stream ranges, a over count_a streams and b over count_b, merged into the result of count_a + count_b
 * streams:  out[i] = ((float)count_a * a[i] + (float)count_b * b[i]) / (float)(count_a + count_b)  in float, every operation
 * rounded on its own; the same rule for frames and for moment films.  `values` floats each (pixels * 3); out may be a or b.
 * What later launches and other devices need (first_stream exists for the same reason).  Against one reduce over the whole range
 * the merge differs by the rounding of another order of sums, a few ulp where no cancellation occurs.  Refused: a NULL pointer,
 * values == 0, count_a + count_b == 0.  The host form computes the same bits on the CPU and needs no device. */
wpt_status wpt_postproc_merge_means(const float* a_device, uint32_t count_a, const float* b_device, uint32_t count_b, uint64_t values,
        float* out_device, void* hip_stream);
wpt_status wpt_postproc_merge_means_host(const float* a_host, uint32_t count_a, const float* b_host, uint32_t count_b, uint64_t values,
        float* out_host);

/* How to split a frame of `pixels` pixels and samples_sqrt^2 samples per pixel for a device that holds `lanes` lanes in flight
 * (wpt_device_lanes): *stream_count = k^2 streams of *stream_samples_sqrt = samples_sqrt / k, where k is a divisor of samples_sqrt
 * that leaves a stream at least 2 x 2 strata (or 1).  Among those in increasing order the first with k^2 * pixels >= 4 * lanes,
 * otherwise the largest.  The total sample count is kept exactly, and the stream count is a square (see the denoiser above).
 * 4 pixels per lane is where a batch of views is near its full rate (profiles/views_rate.txt, profiles/streams_rate.txt).
 * A pure function that needs no device.  Refused: a zero or NULL argument. */
wpt_status wpt_split_plan(uint64_t pixels, uint32_t samples_sqrt, uint32_t lanes, uint32_t* stream_count, uint32_t* stream_samples_sqrt);
/* *lanes = compute units * 1024 of HIP device `device` (wpt_slices_plan's lanes_at_once): what wpt_split_plan is to be given */
wpt_status wpt_device_lanes(int device, uint32_t* lanes);

/* ---- adaptive sampling ----
 * A sample-count map gives every pixel its own count: uint16_t n_p per pixel, [height][width], row 0 = bottom.  A pixel with
 * n_p > 0 is rendered with n_p^2 samples (strata s % n_p, s / n_p) and its value is bit-identical to the plain render with
 * samples_sqrt = n_p; a pixel with n_p = 0 is not rendered, and its entries in the frame and the moment film are not written
 * (a region of interest rendered into an existing frame is a map with zeros outside it).  Every 16-bit value is valid.
 * The moment film (may be NULL): float[height][width][3]; entry c of pixel p is 1 / n_p^2 times the fp32 sum, in sample order,
 * of S_k,c * S_k,c, where S_k,c is the fp32 sum of what sample k added to channel c of the pixel's accumulator (behind the
 * distance and path-length gates).  At n_p = 1 it is frame * frame bit for bit; asking for it changes no bit of the frame.
 * The variance of the pixel's mean is estimated by (moment - frame^2) * N / (N - 1) / N with N = n_p^2.
 * Rendered by the single kernel in one pass (never in the wavefront form), the costly pixels handed out first.  Refused with
 * WPT_ERR_INVALID_ARGUMENT before a device is needed: a NULL map or frame, a width or height of 0 or above 65535, and a block
 * outside the frame. */

/* Asynchronous on `hip_stream`.  `samples_sqrt_device`, `frame_device` and `moments_device` are FULL frames in device
 * memory; only the block's pixels with n_p > 0 are written. */
wpt_status wpt_render_adaptive_block_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_device /* [height][width] */,
        uint32_t block_start, uint32_t block_size, float* frame_device, float* moments_device /* may be NULL */,
        void* hip_stream);

/* Synchronous form with MPICoordinator::submitBlock semantics: `samples_sqrt_host` is the FULL map in host memory,
 * `block_rgb` and `block_moments` (may be NULL) block_size*3 floats each in host memory.  The entries of pixels with n_p = 0
 * are left as the caller had them. */
wpt_status wpt_render_adaptive_block(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params,
        uint32_t width, uint32_t height, const uint16_t* samples_sqrt_host /* [height][width] */,
        uint32_t block_start, uint32_t block_size, float* block_rgb, float* block_moments /* may be NULL */);

/* ---- a frame in resumable stages (progressive sessions) ----
 * A session renders the block's pixels of one frame in stages: every stage renders further rows of strata of every pixel, in
 * one launch of the kernel that a plain wpt_render_block_device of the frame would take (never the wavefront form, the twin
 * that hands pixels out in slices, or the two passes, whatever wpt_set_wavefront and wpt_set_slices say).  A pixel's samples
 * stay one sequence from one generator: between stages a pixel carries on 32 bytes, its generator and its sums with the next
 * stratum, so the finished frame is bit-identical to the one-shot launch however the rows are cut into stages, and a saved
 * and restored session goes on to the same bits.  The first stage hands the pixels out in the frame's order; later stages in
 * the frame's order again (scene in LDS) or the 8x8 tiles that took the stage before longest first (scene in HBM).
 * A preview after r of samples_sqrt rows is (1.0f / (float)(r * samples_sqrt)) * sum per channel: the mean over the strata
 * rendered so far, which are the lower r / samples_sqrt of every pixel's strata -- a picture to look at, not an estimate of
 * the frame.  The preview of a finished session is its frame bit for bit, and that of a session without a stage is 0.
 * Moving scenes, exposure intervals, measured BRDFs, lens cameras, scenes in LDS and in HBM are all covered.  Not covered,
 * and refused with WPT_ERR_UNSUPPORTED (wpt_progress_covers has the messages): counting launches, bands, the transient film,
 * batches of views, adaptive maps and the time-of-flight sensor.
 * A session holds 40 bytes of device memory per pixel (carry 32, time of the last stage 4, order 4) from wpt_progress_begin to
 * wpt_progress_end, allocated with hipMalloc.  All calls on one session are ordered on the streams they are given: use one
 * stream for a session, or synchronise between the streams.  Sessions of one scene on different streams may run side by side.
 * A session reads the scene's device memory in every stage: the wpt_scene must outlive it (wpt_progress_end before
 * wpt_scene_free), and its calls are made with the scene's device current.
 *
 * A saved state is a header of WPT_PROGRESS_HEADER_BYTES bytes, little-endian, then the carry of the block's pixels:
 *   offset   0  uint32  magic, WPT_PROGRESS_MAGIC ("WPTP")
 *            4  uint32  format version, WPT_PROGRESS_STATE_VERSION
 *            8  uint32  width            12  uint32  height          16  uint32  samples_sqrt
 *           20  uint32  block_start      24  uint32  block_size      28  uint32  rows_done
 *           32  uint64  tag: the caller's fingerprint of the scene; the library stores and compares it, nothing more
 *           40  wpt_camera (140 bytes)  180  wpt_params (40 bytes)  220  uint32  reserved, 0
 *          224  block_size records of 32 bytes, pixel block_start first: uint32[4] the pixel's generator, then float[3] the
 *               pixel's sums per channel and uint32 its next stratum i | j << 16.  With rows_done == 0 a record is zeros; with
 *               rows_done == samples_sqrt its three floats are the finished pixel's values (the sums times 1 / samples, as the
 *               kernel wrote them to the frame), so that a finished state still yields its frame: the launch that renders a
 *               pixel's last row writes the frame and stores no carry, so the session copies the block's pixels back from the
 *               frame, and the generator's four words of such a record are stale (those of the stage before, or zeros).
 * wpt_progress_state_info checks a state (sizes against `bytes` before anything is read, then magic, version, ranges, block
 * within width * height, rows_done <= samples_sqrt, the reserved word, the exact length) and needs no device; wurblpt_amd/csrc/wpt_progress_state.h
 * is that parser on its own. */
#define WPT_PROGRESS_MAGIC 0x50545057u
#define WPT_PROGRESS_STATE_VERSION 1u
#define WPT_PROGRESS_HEADER_BYTES 224u
typedef struct wpt_progress wpt_progress; /* opaque session */
typedef struct wpt_progress_info {
    uint32_t version, width, height, samples_sqrt, block_start, block_size, rows_done, reserved;
    uint64_t tag;
    uint64_t state_bytes; /* header and carry */
} wpt_progress_info;

/* WPT_OK if sessions cover such a launch, else WPT_ERR_UNSUPPORTED with the reason.  sensor: as for wpt_kernel_choice (0 one
 * frame, 1 transient film, 2 batch of views, 3 adaptive map, 4 time of flight); counting: the launch counts its work; bands: it
 * renders interleaved bands.  A pure function that needs no device; wpt_progress_begin is sensor 0 without counters or bands. */
wpt_status wpt_progress_covers(uint32_t sensor, uint32_t counting, uint32_t bands);
/* Starts a session for pixels [block_start, block_start + block_size) of a width x height frame; camera and params are copied.
 * WPT_ERR_NO_DEVICE where there is no device, before anything else is looked at. */
wpt_status wpt_progress_begin(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        uint32_t samples_sqrt, uint32_t block_start, uint32_t block_size, uint64_t tag, wpt_progress** out_progress);
/* Renders up to `rows` further rows of strata of every pixel of the block (clamped to what is left), asynchronously on
 * `hip_stream`.  The stage that reaches samples_sqrt writes the block's pixels of `frame_device`, the FULL frame as for
 * wpt_render_block_device; earlier stages do not touch it, and it may be NULL for them.  Refused with
 * WPT_ERR_INVALID_ARGUMENT before anything is launched: rows == 0, a finished session, a NULL frame on the finishing stage.
 * wpt_kernel_name reports the kernel's usual name and wpt_last_render_passes 1. */
wpt_status wpt_progress_advance_device(wpt_progress* progress, uint32_t rows, float* frame_device, void* hip_stream);
/* Synchronous form: the finishing stage writes block_size*3 floats to host memory `block_rgb` as wpt_render_block does; earlier
 * stages do not touch it, and it may be NULL for them. */
wpt_status wpt_progress_advance(wpt_progress* progress, uint32_t rows, float* block_rgb);
uint32_t wpt_progress_rows_done(const wpt_progress* progress);  /* 0 for NULL */
uint32_t wpt_progress_rows_total(const wpt_progress* progress); /* samples_sqrt; 0 for NULL */
/* Writes the preview of the block's pixels into `frame_device`, the FULL frame; pixels outside the block are not written.
 * Asynchronous on `hip_stream`. */
wpt_status wpt_progress_preview_device(wpt_progress* progress, float* frame_device, void* hip_stream);
/* Synchronous form: block_size*3 floats for the block's pixels to host memory `block_rgb`, as wpt_render_block lays them out. */
wpt_status wpt_progress_preview(wpt_progress* progress, float* block_rgb);
/* Frees the session's device memory after its last stream has finished.  NULL is allowed. */
void wpt_progress_end(wpt_progress* progress);
/* The state: its size, the state itself into `bytes` == that size of host memory (waits for the stream of the session's last
 * call), and a new session from it.  wpt_progress_restore compares the state's tag, camera and params with its arguments, the
 * structs bytewise, and names the first that differs in wpt_last_error (WPT_ERR_INVALID_ARGUMENT); a state that
 * wpt_progress_state_info refuses is refused with that message, and so is one with a record whose next stratum is not
 * rows_done << 16 (a damaged body), all before anything is allocated.  The frame's size, samples_sqrt and the block are the
 * state's own: a caller that expects particular ones compares them with wpt_progress_state_info's. */
wpt_status wpt_progress_state_bytes(const wpt_progress* progress, uint64_t* bytes);
wpt_status wpt_progress_save(wpt_progress* progress, void* buffer_host, uint64_t bytes);
wpt_status wpt_progress_restore(wpt_scene* scene, const void* buffer_host, uint64_t bytes, const wpt_camera* camera,
        const wpt_params* params, uint64_t tag, wpt_progress** out_progress);
wpt_status wpt_progress_state_info(const void* buffer_host, uint64_t bytes, wpt_progress_info* info);

/* Waits for the device; WPT_ERR_HIP if a launch since the last call failed (the kernels have no waits that could run
 * out: every loop of theirs ends with its work; lanes that hand a pixel on between its slices never wait for one another). */
wpt_status wpt_scene_check(wpt_scene* scene);

/* ---- ground truth (GroundTruth / getGroundTruth, wurblpt.hpp:453-769) ----
 * One ray through the centre of every pixel, without pixel jitter or lens sampling; arrays of what its
 * first hit is (zero where nothing is hit, material -1).  Array k is the reference's GroundTruth bit k. */
enum {
    WPT_GT_WORLD_SPACE_POSITIONS = 0,          /* 3 floats per pixel */
    WPT_GT_WORLD_SPACE_GEOMETRY_NORMALS = 1,   /* 3 */
    WPT_GT_WORLD_SPACE_GEOMETRY_TANGENTS = 2,  /* 3 */
    WPT_GT_WORLD_SPACE_MATERIAL_NORMALS = 3,   /* 3: after the material's normal map */
    WPT_GT_WORLD_SPACE_MATERIAL_TANGENTS = 4,  /* 3 */
    WPT_GT_CAMERA_SPACE_POSITIONS = 5,         /* 3 */
    WPT_GT_CAMERA_SPACE_GEOMETRY_NORMALS = 6,  /* 3 */
    WPT_GT_CAMERA_SPACE_GEOMETRY_TANGENTS = 7, /* 3 */
    WPT_GT_CAMERA_SPACE_MATERIAL_NORMALS = 8,  /* 3 */
    WPT_GT_CAMERA_SPACE_MATERIAL_TANGENTS = 9, /* 3 */
    WPT_GT_CAMERA_SPACE_DEPTHS = 10,           /* 1: -z of the camera space position */
    WPT_GT_CAMERA_SPACE_DISTANCES = 11,        /* 1: its length */
    WPT_GT_TEXCOORDS = 12,                     /* 2 */
    WPT_GT_WORLD_SPACE_OFFSET_TO_PREV = 13,    /* 3: where the hit point of an animated instance is at tPrev / tNext, minus where it is */
    WPT_GT_WORLD_SPACE_OFFSET_TO_NEXT = 14,    /* 3 */
    WPT_GT_CAMERA_SPACE_OFFSET_TO_PREV = 15,   /* 3: from the camera at tPrev / tNext */
    WPT_GT_CAMERA_SPACE_OFFSET_TO_NEXT = 16,   /* 3 */
    WPT_GT_PIXEL_SPACE_OFFSET_TO_PREV = 17,    /* 2: Surround_Off, non-stereoscopic cameras only (camera.hpp:207-208) */
    WPT_GT_PIXEL_SPACE_OFFSET_TO_NEXT = 18,    /* 2 */
    WPT_GT_MATERIALS = 19,                     /* 1 int32: index into wpt_scene_desc::materials of the hitable's material */
    WPT_GT_ARRAY_COUNT = 20
};
/* components per pixel of array k */
static const uint32_t wpt_gt_components[WPT_GT_ARRAY_COUNT] = { 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 2, 3, 3, 3, 3, 2, 2, 1 };

/* arrays_device[k]: device array of width * height * wpt_gt_components[k] elements (row 0 = bottom), or
 * NULL for an array that is not wanted.  camera_prev / camera_next: the camera at tPrev / tNext (only the
 * transformation is read); NULL = the camera itself.  times: t0, tPrev, tNext for the scene's animated
 * instances (NULL = all zero); the picture is taken at t0.  Asynchronous on `hip_stream`. */
wpt_status wpt_ground_truth_device(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_device[WPT_GT_ARRAY_COUNT], void* hip_stream);
/* The same into host arrays (synchronous). */
wpt_status wpt_ground_truth(wpt_scene* scene, const wpt_camera* camera, const wpt_camera* camera_prev,
        const wpt_camera* camera_next, const float times[3], const wpt_params* params, uint32_t width, uint32_t height,
        void* const arrays_host[WPT_GT_ARRAY_COUNT]);

/* ---- output side (postproc.hpp:44-108): per-pixel operations on a rendered frame ----
 * Device forms work on `pixels` RGB triples in device memory on `hip_stream`.
 *   to_srgb                          linear RGB float -> sRGB uint8 (values above 1 clipped), toSRGB()
 *   max_luminance                    largest CIE Y of the frame, maxLuminance() (synchronises)
 *   uniform_rational_quantization    Schlick's operator on Y, chromaticity kept
 *   scale_luminance                  Y * factor, clamped to 100 * clamp if clamp > 0 */
wpt_status wpt_postproc_to_srgb(const float* rgb_device, uint8_t* srgb_device, uint64_t pixels, void* hip_stream);
wpt_status wpt_postproc_max_luminance(const float* rgb_device, uint64_t pixels, float* result_host, void* hip_stream);
wpt_status wpt_postproc_uniform_rational_quantization(const float* rgb_device, float* out_device, uint64_t pixels,
        float max_val, float brightness, void* hip_stream);
wpt_status wpt_postproc_scale_luminance(const float* rgb_device, float* out_device, uint64_t pixels, float factor,
        float clamp, void* hip_stream);
/* The same for host buffers (upload, run, download): op 0 = to_srgb (out: uint8), 1 = uniform rational
 * quantization (a = max_val, b = brightness; out: float), 2 = scale luminance (a = factor, b = clamp; out:
 * float), 3 = max luminance (out: one float). */
wpt_status wpt_postproc_host(int op, const float* rgb_host, void* out_host, uint64_t pixels, float a, float b);

/* ---- denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with the variance guidance of SVGF (Schied et
 * al. 2017), spatial only ----
 * Filters a rendered frame with what the library already produces beside it: the moment film and the sample-count map of an
 * adaptive render (wpt_render_adaptive_block*) and three arrays of the first-hit pass (wpt_ground_truth*) at the frame's size.
 * All arrays are [height][width][c], row 0 = bottom:
 *   frame, moments    3 floats per pixel                       samples_sqrt   n_p, one uint16 per pixel
 *   positions         WPT_GT_CAMERA_SPACE_POSITIONS (P)        normals        WPT_GT_CAMERA_SPACE_MATERIAL_NORMALS (n)
 *   materials         WPT_GT_MATERIALS (m; -1 where the ray hit nothing)
 * Preparation: per channel v = max(moment - frame * frame, 0) / (float)(n_p * n_p - 1) where n_p >= 2, else frame * frame;
 * Y(c) = (kr * r + kg * g) + kb * b with the Y row of the RGB -> XYZ matrix; V_0 = Y(sqrt(v))^2, the variance of the luminance.
 * Iteration i = 0 .. iterations - 1 with step s = 2^i reads the 5 x 5 taps q = p + s * (dx, dy) with the B3 weights
 * h = (1, 4, 6, 4, 1) / 16, dy outer, dx inner; taps outside the frame and taps with m(q) != m(p) are skipped:
 *   L   = sigma_l * sqrt(g) + 1e-10f,  g the (1,2,1) x (1,2,1) mean of V_i over the in-frame neighbours at unit offsets
 *   w_n = max(0, n(p) . n(q)) squared normal_log2 times;  D = P(q) - P(p), t = n(p) . D, dd = D . D,
 *   e_z = dd == 0 ? 0 : (t * t) / ((sigma_z * sigma_z) * dd)      (w_n = 1 and e_z = 0 where m(p) < 0)
 *   e_l = |Y(c_i(q)) - Y(c_i(p))| / L,   w = (h[dy] * h[dx]) * w_n * expf(-(e_z + e_l)),  the centre tap's w = 9/64
 *   c_{i+1}(p) = sum(w * c_i(q)) / sum(w),   V_{i+1}(p) = sum((w * w) * V_i(q)) / (sum(w) * sum(w))
 * in float, in tap order, every operation rounded on its own.  `out`: the filtered frame; `variance` (may be NULL): V after the
 * last iteration, one float per pixel.  iterations = 0 copies the frame.  The inputs must be finite and are never written.
 * Refused with WPT_ERR_INVALID_ARGUMENT before a device is needed: a NULL input or `out`, a width or height of 0 or above
 * 65535, iterations > WPT_DENOISE_MAX_ITERATIONS, normal_log2 > WPT_DENOISE_MAX_NORMAL_LOG2, a sigma that is not finite and
 * positive, an output that overlaps an input or the other output.
 * The device form is asynchronous on `hip_stream`; its scratch (64 bytes per pixel) is allocated and freed in stream order.
 * The host form computes the same bits on the CPU and needs no device. */
#define WPT_DENOISE_MAX_ITERATIONS 8u
#define WPT_DENOISE_MAX_NORMAL_LOG2 16u
typedef struct wpt_denoise_params {
    float sigma_l;        /* default 1: how many standard deviations of luminance a tap may differ by.  Schied et al. publish 4; on the
                           * Cornell box at 16 spp that doubles the error against a converged render, 1 lowers it by 3.5 % at
                           * 64 x 64 and by 20 % at 256 x 256 (profiles/denoise_quality.txt) */
    float sigma_z;        /* default 0.1: the sine of the angle by which a tap may leave the pixel's tangent plane */
    uint32_t normal_log2; /* default 7: the normal weight is the cosine to the power 2^7 = 128 (Schied et al.) */
    uint32_t iterations;  /* default 5, 0 .. WPT_DENOISE_MAX_ITERATIONS */
} wpt_denoise_params;
/* `params` NULL: the defaults */
wpt_status wpt_postproc_denoise(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_device, float* variance_device, void* hip_stream);
wpt_status wpt_postproc_denoise_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, uint32_t width, uint32_t height,
        const wpt_denoise_params* params, float* out_host, float* variance_host);
/* "tile" (a workgroup's pixels and their halo in LDS) or "gather" (taps from device memory): the form the device's iteration
 * with this step takes, decided from the step alone; both give the same bits */
const char* wpt_postproc_denoise_form(uint32_t step);

/* ---- first-hit colours: what the surface behind a pixel's centre multiplies the light with, and what it emits itself ----
 * One ray per pixel, exactly the ray of wpt_ground_truth*: pixel centre, no jitter, lens radius 0, time params->t0 (animated
 * instances, spheres and lens distortion are followed).  All arrays are [height][width][c], row 0 = bottom; any may be NULL:
 *   albedo    3 floats per pixel          emission  3 floats per pixel
 *   guide[0]  WPT_GT_CAMERA_SPACE_POSITIONS, guide[1]  WPT_GT_CAMERA_SPACE_MATERIAL_NORMALS, guide[2]  WPT_GT_MATERIALS (int32):
 *             bit for bit what wpt_ground_truth_device writes for times[0] = params->t0 (`guide` itself may be NULL: none wanted)
 * The colours look through WPT_MAT_TWOSIDED as the path tracer does (the back child sees the hit from its front); for the
 * material m they arrive at, with `d` the ray's direction:
 *   emission  rgb of Material::emitted(m, hit, d): diffuse and spot lights (cone, texture), ModPhong's emissive term; the rgb of
 *             a time-of-flight light is 0.  No hit: the rgb of the environment map along d, +0 without one.
 *   albedo    back side: +0, except GLASS.  Front side: LAMBERTIAN, GGX, MIRROR, MODPHONG the rgb of tex[0] / v[0] (albedo, F0,
 *             mirror colour, diffuse colour: what the kind multiplies the throughput with); GLASS (both sides) and RGL (1, 1, 1);
 *             NONE, LIGHT_DIFFUSE, LIGHT_SPOT and no hit +0.  ModPhong's specular colour v[1] is not part of it.
 * Refused with WPT_ERR_INVALID_ARGUMENT before a device is needed: a NULL scene, camera or params, a width or height of 0 or
 * above 65535, all five outputs NULL, outputs that overlap.  The device form is asynchronous on `hip_stream`. */
wpt_status wpt_first_hit_colours_device(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width,
        uint32_t height, float* albedo_device, float* emission_device, void* const guide_device[3], void* hip_stream);
/* The same into host arrays (synchronous). */
wpt_status wpt_first_hit_colours(wpt_scene* scene, const wpt_camera* camera, const wpt_params* params, uint32_t width, uint32_t height,
        float* albedo_host, float* emission_host, void* const guide_host[3]);

/* ---- the denoiser on the demodulated frame: the surface's own colours are taken out before the filter and put back after it,
 * so that a texture is not filtered with the noise ----
 * `albedo`, `emission`: the planes of wpt_first_hit_colours* at the frame's size; everything else as for wpt_postproc_denoise.
 * `albedo_floor` <= 0: the default 1.0f / 64.  Per pixel and channel c, every operation rounded on its own:
 *   d_c = albedo_c >= albedo_floor ? albedo_c : 1.0f            u_c = (frame_c - emission_c) / d_c
 *   v_c = n_p >= 2 ? v(frame_c, moment_c, n_p) / (d_c * d_c) : u_c * u_c        (v: the channel variance of the plain form)
 *   the filter's colour record is (u_r, u_g, u_b, Y(sqrt(v))^2); the guide and the iterations are those of the plain form
 *   out_c = c_c * d_c + emission_c after the last iteration (iterations = 0: u_c * d_c + emission_c)
 * u may be negative where a lamp covers a pixel's centre but not all of its footprint.  `variance` (may be NULL): V of the
 * DEMODULATED luminance after the last iteration, in the units of u, not of the frame.
 * Refused as wpt_postproc_denoise is, and for a NULL albedo or emission and an albedo_floor that is NaN or infinite. */
wpt_status wpt_postproc_denoise_demodulated(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device, const float* albedo_device,
        const float* emission_device, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_device, float* variance_device, void* hip_stream);
wpt_status wpt_postproc_denoise_demodulated_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, const float* albedo_host,
        const float* emission_host, uint32_t width, uint32_t height, const wpt_denoise_params* params, float albedo_floor,
        float* out_host, float* variance_host);

/* ---- temporal accumulation: a pixel's estimate carried from frame to frame along the scene's motion, in front of the denoiser ----
 * Frame f of a sequence is rendered with its own sample streams (wpt_render_split*, first_stream = f * K), so that frames are
 * independent estimates; where a surface stays visible, F frames of n samples then count as F * n samples before the spatial
 * filter runs.  A HISTORY is the denoiser's own three 16-byte records per pixel, kept: [3][height][width] records of four floats
 * (WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL bytes per pixel), row 0 = bottom,
 *   plane 0 (A)  P.xyz and the bits of m                         plane 1 (B)  n.xyz and the history length N as a float
 *   plane 2 (C)  the accumulated rgb and V, the variance of its luminance
 * Callers may read and build histories.  wpt_postproc_temporal_accumulate writes a new history from the current frame and the
 * previous one; wpt_postproc_denoise_history runs the denoiser's iterations on a history as it is.
 * Inputs as for wpt_postproc_denoise, and the two motion arrays of wpt_ground_truth* at the frame's size:
 *   pixel_offset_to_prev   WPT_GT_PIXEL_SPACE_OFFSET_TO_PREV (dx, dy), from pixel centre to pixel centre, in pixels
 *   camera_offset_to_prev  WPT_GT_CAMERA_SPACE_OFFSET_TO_PREV (3 floats)
 * both NULL: the caller declares the scene and the camera at rest.  For pixel p = (x, y) the preparation of the denoiser gives
 * the current records A = (P, m), B = (n, .) and C = (rgb, V_cur); the new records are A, B' and C'.  In float, every operation
 * rounded on its own, in this order:
 *   history_prev == NULL (the first frame): C' = C, B'.w = 1.
 *   Source of the history.  Both offset arrays NULL: the single tap (x, y) with weight 1, and E = P.  Otherwise, m < 0 (nothing
 *   hit; the ground truth pass writes offset 0 there): reset.  Otherwise fx = (float)x + dx, fy = (float)y + dy;
 *   !(fx > -1 && fx < width && fy > -1 && fy < height): reset (NaN too).  ix = floorf(fx), wx1 = fx - ix, wx0 = 1 - wx1, the same
 *   for y; the taps are (ix + i, iy + j), j outer, i inner, with the weights w = wy_j * wx_i; E = P + camera_offset_to_prev[p],
 *   the point as the previous camera saw it.
 *   A tap q counts if its weight is not 0, it lies in the frame, m_q == m and, for m >= 0, n . n_q >= normal_cos_min and with
 *   D = P_q - E: D . D <= (tol * tol) * (E . E), tol = position_tolerance.  (A tap of weight 0 is never read, so whole-pixel
 *   shifts are exact.)  No tap counts: reset, C' = C, B'.w = 1.
 *   Otherwise sw = sum(w), H = sum(w * C_q.rgb) / sw, V_H = sum(w * C_q.w) / sw, N_H = sum(w * B_q.w) / sw;
 *   N' = min(N_H + 1, max_history), a = 1 / N', b = 1 - a;  C'.rgb = b * H + a * C.rgb,  C'.w = (b * b) * V_H + (a * a) * V_cur
 *   (the variance of a weighted mean of independent estimates),  B'.w = N'.
 *   A pixel the current frame did not sample (samples_sqrt[p] == 0): with a counting tap C' = (H, V_H) and B'.w = N_H, the history
 *   carried over; without one C' = C and B'.w = 0, so that the next sampled frame replaces it entirely.
 * The normals compared are camera-space normals of two different frames: a camera that turns between frames turns a static
 * surface's normal with it, and normal_cos_min has to cover that turn.  Lighting that changes between frames is not detected;
 * max_history is the only guard.  `length_out` (may be NULL): B'.w, one float per pixel.
 * Refused with WPT_ERR_INVALID_ARGUMENT before a device is needed: a NULL frame, moments, samples_sqrt, positions, normals,
 * materials or history_out; a width or height of 0 or above 65535; exactly one of the two offset arrays NULL; history_out that
 * is or overlaps history_prev (taps gather from neighbours: nothing works in place); max_history not finite or below 1;
 * normal_cos_min outside [-1, 1]; position_tolerance negative or not finite; reserved != 0.  The inputs must be finite, except
 * the offsets, which may be anything.  The device form is one launch, asynchronous on `hip_stream`, and takes no scratch.  The
 * host form computes the same bits on the CPU and needs no device. */
#define WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL 48u
typedef struct wpt_temporal_params {
    float max_history;        /* default 32: the longest history length, in frames */
    float normal_cos_min;     /* default 0.9: the smallest accepted cosine between the current and the tap's normal */
    float position_tolerance; /* default 0.02: relative to the distance from the previous camera */
    uint32_t reserved;        /* must be 0 */
} wpt_temporal_params;
/* `params` NULL: the defaults */
wpt_status wpt_postproc_temporal_accumulate(const float* frame_device, const float* moments_device, const uint16_t* samples_sqrt_device,
        const float* positions_device, const float* normals_device, const int32_t* materials_device,
        const float* pixel_offset_to_prev_device, const float* camera_offset_to_prev_device, const void* history_prev_device,
        uint32_t width, uint32_t height, const wpt_temporal_params* params, void* history_out_device, float* length_out_device,
        void* hip_stream);
wpt_status wpt_postproc_temporal_accumulate_host(const float* frame_host, const float* moments_host, const uint16_t* samples_sqrt_host,
        const float* positions_host, const float* normals_host, const int32_t* materials_host, const float* pixel_offset_to_prev_host,
        const float* camera_offset_to_prev_host, const void* history_prev_host, uint32_t width, uint32_t height,
        const wpt_temporal_params* params, void* history_out_host, float* length_out_host);
/* The denoiser's iterations (wpt_postproc_denoise above) on a history: guide and colours are the history's planes, there is no
 * preparation; on the history of a first frame the result is wpt_postproc_denoise's of the same inputs, bit for bit.
 * iterations = 0 unpacks the accumulated frame and its variance, which is how a caller reads them.  The history is never
 * written.  `variance` may be NULL.  Refused as wpt_postproc_denoise is (a NULL history or `out`, the sizes, the parameters,
 * outputs that overlap the history or each other).  The device form is asynchronous on `hip_stream`; its scratch (32 bytes per
 * pixel, none with no iterations) is allocated and freed in stream order. */
wpt_status wpt_postproc_denoise_history(const void* history_device, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float* out_device, float* variance_device, void* hip_stream);
wpt_status wpt_postproc_denoise_history_host(const void* history_host, uint32_t width, uint32_t height, const wpt_denoise_params* params,
        float* out_host, float* variance_host);

/* ---- image operations (postproc.hpp:112-309): scale(), applyLensDistortion() / distort() / undistort(), despeckle(),
 * cameraSpaceDistanceToCoords() and cameraSpaceToPMDSpace() ----
 * Images are [height][width][components] floats, row 0 = bottom; every product and sum is rounded on its own; the device form,
 * the host form and the reference's function give the same bits.
 * Sampling rule of resample, lens_warp and distance_to_coords (texture_image.hpp:182-212, float data, no sRGB): uv = tc - floor(tc)
 * (coordinates outside [0, 1) wrap); uvs = max(0, uv.s * width - 0.5f), x0 = (size_t)uvs, x1 = x0 + 1, both clamped to width - 1,
 * alpha = uvs - x0, the same for t; value = mix(mix(v00, v10, alpha), mix(v01, v11, alpha), beta), mix(x, y, a) = x + a * (y - x).
 * A texel is expanded by the component count first (texture_image.hpp:152-177): 3 -> (r, g, b, 1), 4 -> unchanged, 1 -> (v, v, v, 1),
 * 2 -> (v0, v0, v0, v1), and output component c is component c of the expansion.  OUTPUT COMPONENT 1 OF A TWO-COMPONENT IMAGE IS
 * THEREFORE COMPONENT 0's VALUE: the reference's functions return that, and it is kept.
 * A sampling coordinate that is not finite (undefined in the reference) makes every component of that output pixel +0.
 *   resample             pixel (x, y) of the new_width x new_height output samples at ((x + 0.5f) / new_width, (y + 0.5f) / new_height)
 *   lens_warp            p = (x + 0.5f) * (1.0f / width), q likewise; forward != 0 (an undistorted render becomes what the lens
 *                        shows): LensDistortion::undistort with the image's width and height, else LensDistortion::distort; then
 *                        sampled there.  WPT_DISTORTION_NONE resamples at the pixel centres like every other type.
 *   despeckle            RGB only.  The 3 x 3 neighbourhood with coordinates clamped to the frame, sorted by luminance (the Y of
 *                        max_luminance), equal luminances in the neighbourhood's row-major order; the pixel is replaced by sorted
 *                        element 4 where its luminance is >= element 8's and >= min_factor * element 7's.  Inputs must be finite.
 *   distance_to_coords   distance = component 0 of the image at LensDistortion::distort(p, q); uv = ((p, q) - dist_center) *
 *                        dist_inverse_focal_length; xyz = (vec3(uv, 1) / length(vec3(uv, 1))) * distance; the output is three
 *                        floats (x, y, -z), and with pmd_space != 0 (x, -y, z): the PMD camera's coordinate system.
 * Of `camera` only distortion_type, k1 .. p2, b1 .. b4 and the three dist_* pairs are read.
 * All forms refuse with WPT_ERR_INVALID_ARGUMENT before a device is needed: a NULL pointer, a width or height (of the image or of
 * the output) of 0 or above 65535, a component count outside 1 .. 4 (despeckle: other than 3), an unknown distortion type, a
 * min_factor that is not finite, an output that overlaps the image.
 * The device forms are asynchronous on `hip_stream`, one launch each, and take no scratch; the host forms need no device. */
wpt_status wpt_postproc_resample(const float* image_device, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_device, void* hip_stream);
wpt_status wpt_postproc_resample_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, uint32_t new_width,
        uint32_t new_height, float* out_host);
wpt_status wpt_postproc_lens_warp(const float* image_device, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_device, void* hip_stream);
wpt_status wpt_postproc_lens_warp_host(const float* image_host, uint32_t width, uint32_t height, uint32_t components, const wpt_camera* camera,
        int forward, float* out_host);
wpt_status wpt_postproc_despeckle(const float* rgb_device, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_device, void* hip_stream);
wpt_status wpt_postproc_despeckle_host(const float* rgb_host, uint32_t width, uint32_t height, uint32_t components, float min_factor,
        float* out_host);
wpt_status wpt_postproc_distance_to_coords(const float* distances_device, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_device, void* hip_stream);
wpt_status wpt_postproc_distance_to_coords_host(const float* distances_host, uint32_t width, uint32_t height, uint32_t components,
        const wpt_camera* camera, int pmd_space, float* coords_host);
/* "tile" (a workgroup's pixels and the ring around them in LDS) or "gather" (nine loads per lane): the form the device's
 * despeckle takes; both give the same bits */
const char* wpt_postproc_despeckle_form(void);
/* A PROCESS-GLOBAL hook for tests and measurements like wpt_set_launch_config: -1 = the form the library was built with, 0 =
 * gather, 1 = tile.  Results do not depend on it. */
wpt_status wpt_set_despeckle_form(int form);
/* the output pixels of one workgroup of the device forms (for tests of sizes around it) */
void wpt_postproc_image_ops_tile(uint32_t* width, uint32_t* height);

/* Kernel launch geometry knobs (0 = default); for benchmarking only, results do not change.  wpt_set_launch_config,
 * wpt_set_top_nodes and wpt_set_wavefront are PROCESS-GLOBAL hooks for tests and measurements: set them before rendering
 * starts, not while other threads render (MPICoordinator's worker threads read them).
 * variant, byte 0: 0x01 scene from HBM even if it fits LDS, 0x02 all-features kernel, 0x20 separate SHADE / NEE-END / NEW rounds, 0x10 no pixel pool (every lane renders the one pixel it was launched for), 0x80 material records from HBM even where they fit into LDS next to the scene, 0x40 never two passes over a frame (timed first row of strata, then the rest with the longest tiles first; scenes fetched from HBM) and never pixels in slices (wpt_set_slices; scenes in LDS), bits 0x0c: a kind of material with few lanes in a long round stands back once (0 = fewer than 6 lanes, 0x04 = never, 0x08 = fewer than 3, 0x0c = fewer than 12; kernels without textures / spheres / environment only); byte 1: leave threshold of the traversal loop in eighths + 1; byte 2: lanes a long round needs + 1; byte 3:
 * leaf bias (DESIGN.md section 4 has what each was measured to do). */
wpt_status wpt_set_launch_config(uint32_t threads_per_group, uint32_t variant);
/* Storage order of the BVH nodes in HBM for scenes uploaded from now on: the first `nodes` nodes of a tree that is
 * larger than an L2 slice are stored level by level in front of the array, the subtrees below them depth-first
 * (0 = the whole tree depth-first, the reference's own array order; default 65536 = 2 MiB).  Visiting order and results do
 * not depend on it. */
wpt_status wpt_set_top_nodes(uint32_t nodes);
/* How rays walk the tree (results do not depend on it; process-global like the hooks above, set it before uploading and
 * rendering, not while other threads render):
 *   WPT_WALK_WIDE           scenes uploaded from now on also get the tree collapsed by one level (128-byte nodes that hold the
 *                           boxes of a node's four grandchildren), and product launches that fetch the scene from HBM walk that:
 *                           four box tests per fetch, leaf tests in BVH::hit's order (bvh.hpp:277-311), the same hits bit for bit
 *                           (wpt_pathtrace.inc.h says why; rays for which the argument does not hold walk the binary tree).
 *                           Trees with a non-finite box, a child's box outside its parent's, or a worst case of more than 96
 *                           waiting entries have no wide form and are walked as before.
 *   WPT_WALK_FULL_SHADOW    light rays towards the environment walk the tree to the end like the reference's (product launches
 *                           end such a walk at its first accepted hit: the answer the ray is traced for is known there)
 *   WPT_WALK_COUNT_PRODUCT  counting launches, which otherwise walk like the reference so that their counters are its
 *                           counters, count the product's shortened walks instead
 *   WPT_WALK_TRIANGLES_AS_GIVEN  scenes uploaded from now on keep their triangle records in the caller's order (measurements; by
 *                           default the records are stored in the order of their leaves in the tree, so that a subtree's
 *                           triangles share cache lines)
 *   WPT_WALK_SELECT_CORNERS  plain product launches of the kernel with the scene in LDS keep the triangle test that selects the
 *                           corners' components by the ray's axes (A/B runs and tests; by default such a launch holds the
 *                           corners in LDS in all three rotations of (x, y, z), where that still leaves four workgroups per
 *                           compute unit, and a test reads them in its ray's order: wpt_kernel_form)
 *   WPT_WALK_NO_FOLD        the kernels with the scene in LDS keep every node's own first child in their copy of the tree (A/B
 *                           runs and tests; by default a first child whose box is its parent's bit for bit is folded into the
 *                           parent's link, because its box test repeats the parent's on the same inputs: wpt_fold.h); the
 *                           links that go round nodes are built on the fold, so this flag keeps those away too
 *   WPT_WALK_NO_BYPASS      the kernels with the scene in LDS test every node of the folded tree (A/B runs and tests; by default
 *                           links that lead to an inner node of the scene's plan, wpt_bypass_plan below, lead to its first child)
 *   WPT_WALK_SMALL_WORKGROUPS  launches of the kernel with rotated corners keep its workgroups of 256 lanes (A/B runs and tests;
 *                           by default such a launch runs as one workgroup of 1024 lanes per compute unit with the node array
 *                           in LDS once per sign octant of a ray's direction, so that a box test sorts no slab distances --
 *                           where no box of the tree has a NaN bound or lo > hi and the copies fit the unit's 160 KiB:
 *                           wpt_kernel_workgroup)
 *   WPT_WALK_HIT_DATA_IN_HBM  launches in that form of 1024 lanes fetch a hit's data from global memory like every other kernel
 *                           (A/B runs and tests; by default they keep, behind the node copies and as far as a compute unit's
 *                           LDS has room, a record per triangle with its shading attributes, the hot spots and the instances'
 *                           normal matrices: wpt_kernel_hit_data) */
#define WPT_WALK_WIDE 1u
#define WPT_WALK_FULL_SHADOW 2u
#define WPT_WALK_COUNT_PRODUCT 4u
#define WPT_WALK_TRIANGLES_AS_GIVEN 8u
#define WPT_WALK_SELECT_CORNERS 16u
#define WPT_WALK_NO_FOLD 32u
#define WPT_WALK_NO_BYPASS 64u
#define WPT_WALK_SMALL_WORKGROUPS 128u
#define WPT_WALK_HIT_DATA_IN_HBM 256u
wpt_status wpt_set_walk(uint32_t flags);
/* Nodes whose link the kernels with the scene in LDS fold in their copy of the tree: inner nodes that go past one or more inner
 * first children with their own box.
 *   wpt_scene_folded_links  of an uploaded scene, counted at the upload (0 for a scene that does not fit LDS)
 *   wpt_fold_plan           the same count from a description, a pure function that needs no device, whatever the scene's size;
 *                           lds_words (or NULL): node_count words, word 7 of every node's copy in LDS with the folds applied
 *                           (an index: where a ray that passes the box goes, node_count = out of the tree; >= 2^31: a leaf);
 *                           the words are those of the description's own depth-first order with its own triangle indices */
wpt_status wpt_scene_folded_links(const wpt_scene* scene, uint32_t* folded);
wpt_status wpt_fold_plan(const wpt_scene_desc* desc, uint32_t* folded, uint32_t* lds_words);
/* Inner nodes that the walk of a scene in LDS leaves out (wpt_bypass.h): a node whose children's boxes lie within its own almost
 * always passes its test, and a ray that fails it fails its children as well, so every link that led to it leads to its first
 * child instead -- for rays whose slab distances are numbers; the others, and trees with a NaN bound, walk the fold's links.
 * Which of the eligible nodes go is chosen at the upload by a cost model over a fixed sample of rays made from the scene.
 *   wpt_scene_bypassed_nodes  nodes left out of an uploaded scene's walk (0 for a scene that does not fit LDS)
 *   wpt_bypass_plan           the same count from a description, a pure function that needs no device (0 for a scene that does
 *                             not fit LDS); words (or NULL): 2 * node_count + 1 words -- per node its skip link and word 7 of its
 *                             copy in LDS as wpt_fold_plan gives it, both led past the nodes left out, then the node a ray starts at
 *   wpt_set_bypass            tests: 0 = the cost model chooses (default), 1 = every eligible node is left out; read at the upload
 *                             and by wpt_bypass_plan (process-global like the hooks above) */
wpt_status wpt_scene_bypassed_nodes(const wpt_scene* scene, uint32_t* count);
wpt_status wpt_bypass_plan(const wpt_scene_desc* desc, uint32_t* count, uint32_t* words);
wpt_status wpt_set_bypass(uint32_t mode);
/* Pixels in slices (results do not depend on it; process-global like the hooks above).  A pooled, plain product launch of the
 * kernels with the scene in LDS cuts every pixel into `units` units of `rows` rows of strata and hands out all first units,
 * then all second units, and so on, each time in the frame's own order, in one launch: the work that is left when the pool
 * runs dry is a fraction of a pixel per lane instead of a whole one.  A pixel's samples stay one sequence from one generator
 * (a unit goes on where the one before it stopped), so the frame is the same bit for bit.  Variant bit 0x40 of
 * wpt_set_launch_config switches it off like the two passes of the other kernels; wpt_kernel_form says ", sliced xU".
 *   wpt_slices_plan   the library's own choice for a launch of block_size pixels on a device that holds lanes_at_once lanes
 *                     (compute units * 1024): units = 1 (not sliced) outside 2 to 64 pixels per lane and below samples_sqrt = 8.
 *                     Otherwise it aims for t = samples_sqrt * sqrt(0.5 / pixels per lane) units, 15 at most -- a unit's start
 *                     costs a hand-over through memory, and the end of the launch that the units shorten is the smaller a part
 *                     of it the more pixels a lane renders; below t = 2 the launch is not sliced, otherwise rows =
 *                     ceil(samples_sqrt / t), at least 2, and units = ceil(samples_sqrt / rows).  A pure function of its
 *                     arguments that needs no device.
 *   wpt_set_slices    0 = the plan (default), 1 = never, n = 2 .. 15: rows = ceil(samples_sqrt / n), units = ceil(samples_sqrt /
 *                     rows), whatever the pixels per lane.  WPT_SLICES_DECLINE_ODD beside n (tests): a unit of a pixel on an odd
 *                     slot of the launch is never taken over by the lane that draws it; the lane that rendered the unit before
 *                     it runs it straight on -- the path a launch otherwise takes only where a unit is drawn before it is ready.
 *   wpt_last_slice_stats  of the process's most recent render call, after waiting for the device: units that the lane that drew
 *                     them took over, and units that their pixel's lane ran on with; 0 and 0 if the call was not sliced.  Their
 *                     sum is pixels * (units - 1). */
#define WPT_SLICES_DECLINE_ODD 0x100u
wpt_status wpt_slices_plan(uint32_t block_size, uint32_t lanes_at_once, uint32_t samples_sqrt, uint32_t* units, uint32_t* rows);
wpt_status wpt_set_slices(uint32_t n);
wpt_status wpt_last_slice_stats(uint64_t* taken, uint64_t* continued);
/* Which form of the path tracer renders frames whose scene is fetched from HBM (results do not depend on it):
 * mode 0 = the library decides per launch (default), 1 = the wavefront form wherever it exists (trace and shade as two
 * kernels that hand rays through HBM, wpt_wavefront.inc.h: everything but counting launches and moving scenes), 2 = never.
 * groups, bits 0-7: groups of lanes that iterate on streams of their own (0 = default), bits 8-15 (measurements): workgroups
 * of the trace kernel per compute unit (0 = what fits), bit 16 (measurements): one shade launch per kind of material, so that a
 * kernel trace tells the kinds apart; chunk: queue entries a wave of the trace
 * takes per atomic (0 = default); flags bit 0: the shade walks the ray queue in its own order instead of by kind of
 * material, bits 1-7: nodes in front of the node array that the trace walks from LDS, in units of 128 (0 = default, 0x7f =
 * none), bits 8-13: lanes of a wave that must have finished before the trace deals it new rays (0 = default), bits 16-31: node
 * steps a ray takes per launch of the trace before its walk is suspended until the next (0 = default, 0xffff = no limit).
 * Process-global like wpt_set_launch_config and wpt_set_top_nodes: a hook for tests and measurements, set it before
 * rendering starts, not while other threads render. */
wpt_status wpt_set_wavefront(uint32_t mode, uint32_t groups, uint32_t chunk, uint32_t flags);
/* The library reads no environment variable. */

/* Profiling hook: `stats_device` (device pointer to WPT_SCHED_STATS uint64, or NULL to switch off) receives
 * the wave scheduler's statistics of launches that also count work (counters_device != NULL):
 * [0] NODE rounds [1] NODE loop iterations [2] sum of lanes active in them, then (rounds, lanes)
 * for LEAF [3,4], SHADE [5,6], NEE-END [7,8], NEW [9,10]; shader-clock ticks a wave spent in
 * traversal [11], SHADE [12], NEE-END [13], NEW [14]; [15] unused; [16..23] shader-clock ticks summed
 * over lanes per section of the SHADE block (hit record, scatter, emission, light pdf 1, light sample,
 * light pdf 2, evaluation towards the light, environment sampling / continuation); [24 .. 47] executions of each stretch of
 * the kernel's code by waves (at least one lane ran it) and [48 .. 71] by lanes, in the order of wpt_blocks.h's SEC_* (node step,
 * leaf test, ray start, ...: tools/instruction_budget.py multiplies them with the stretches' instruction counts). */
#define WPT_SCHED_STATS 72
wpt_status wpt_set_scheduler_stats(unsigned long long* stats_device);

/* Kernel family of the process's most recent render call (for profile matching). */
const char* wpt_kernel_name(void);
/* The form of that family's kernel the most recent render call launched, where a family has more than one: "rotated corners" for
 * the kernel with the scene in LDS that holds the corners in all three rotations (WPT_WALK_SELECT_CORNERS above), otherwise ""; ", sliced xU" behind it where the launch handed its pixels out in U units each
 * (wpt_set_slices).  "rotated corners, leaf links from the nodes": that kernel for a scene whose tree does not have exactly one
 * leaf per triangle (the description admits it); its leaf tests read the leaf's node for the skip link, as every other kernel
 * with the scene in LDS does, where otherwise they find it in the triangle's corner records. */
const char* wpt_kernel_form(void);
/* Lanes per workgroup of the path-tracing kernel the most recent render call launched: 256, or 1024 for the large form of the
 * kernel with rotated corners (WPT_WALK_SMALL_WORKGROUPS above).  *ordered_boxes (or NULL): 1 if that launch walked ordered box
 * copies, else 0.  wpt_kernel_name, wpt_kernel_form and wpt_kernel_choice do not tell the two apart: the large form is a
 * decision of the launch on top of that choice. */
uint32_t wpt_kernel_workgroup(uint32_t* ordered_boxes);
/* What of a hit's data the path-tracing kernel of the most recent render call read from LDS instead of global memory: a sum of
 * WPT_HIT_DATA_RECORDS (per triangle the shading attributes and the instance, material and flag words), WPT_HIT_DATA_HOTSPOTS
 * (the hot spots with their faces) and WPT_HIT_DATA_NORMALS (the normal matrices of the instances that transformed triangles
 * name).  The large form of 1024 lanes is built for all three, for the first two and for none, and a launch runs the largest of
 * these whose parts fit in front of its paths' words; 0 for every other kernel and under WPT_WALK_HIT_DATA_IN_HBM.  The frame is
 * the same bit for bit either way. */
#define WPT_HIT_DATA_RECORDS 1u
#define WPT_HIT_DATA_HOTSPOTS 2u
#define WPT_HIT_DATA_NORMALS 4u
uint32_t wpt_kernel_hit_data(void);
/* 1 if the path-tracing kernel of the most recent render call read the material records by LDS address, else 0: a launch in the
 * form of 1024 lanes whose kernel reads hit records and hot spots from LDS keeps the material records there as well -- behind
 * the corners where they are in LDS anyway, else behind that data where they still end in front of the paths' cold words -- and
 * fetches a hit's material with LDS instructions; every other launch reads them through the scene's array.  Not a part of
 * wpt_kernel_hit_data's sum; WPT_WALK_HIT_DATA_IN_HBM switches it off with the parts. */
uint32_t wpt_kernel_materials_in_lds(void);
/* 1 if the path-tracing kernel of the most recent render call read the launch's constants -- the origin of the camera's rays,
 * evaluated once per launch, its frustum and rotation, the reciprocals of the frame's size and of samples_sqrt -- from a record
 * of four quadwords in LDS, else 0: a launch that reads the material records by LDS address has that record in the last
 * quadwords in front of the paths' cold words where the scene ends in front of them; every other launch reads the kernel's
 * arguments per sample.  The words are the same, and so is the frame, bit for bit. */
uint32_t wpt_kernel_launch_record(void);
/* Where such a launch keeps the material records: a pure function that needs no device (tests).  node_count, tri_count,
 * material_count: the scene's tree, triangles and materials; behind_corners: 1 if the kernel choice has the material records in
 * LDS behind the corners anyway (wpt_kernel_choice's materials_in_lds & 1); instance_count: the instances whose normal matrix a
 * transformed triangle names; hotspot_count: the hot spots.  *at (or NULL): the quadword (16 bytes), from the scene's start in
 * LDS, where the records start or would; *quads (or NULL): the quadwords of the scene with everything the launch keeps.
 * Returns 1 if the launch reads them by LDS address, else 0. */
int wpt_material_places(uint32_t node_count, uint32_t tri_count, uint32_t material_count, uint32_t behind_corners, uint32_t instance_count,
        uint32_t hotspot_count, uint32_t* at, uint32_t* quads);
/* Which instantiation of the single kernel renders a launch, from the facts the library decides by: a pure function that needs
 * no device (tests).  need: the feature bits of the scene and the launch's cameras (wpt_device.h, FEAT_*; FEAT_ANIM for a moving
 * scene, a moving camera or an exposure interval); sensor: 0 one frame, 1 transient film, 2 batch of views, 3 adaptive sampling,
 * 4 time of flight; count: the launch counts its work; node_count, tri_count, material_count: the scene's; scene_has_wide: it was
 * uploaded under WPT_WALK_WIDE and has the collapsed tree; variant, walk: the words of wpt_set_launch_config and wpt_set_walk.
 * Results: wpt_kernel_name and wpt_kernel_form (without ", sliced xU") of such a launch, key = the kernel's template arguments
 * { F, COUNT, LDSSCENE, WIDE }, the bytes of LDS behind the paths' own words that the launch asks for (0: the scene is fetched
 * from HBM), and the word of KernelArgs::materialsInLds (1: the material records are in LDS too, 2: the LDS copy of the tree is
 * folded).  WPT_ERR_UNSUPPORTED, with the key in the message, if the library has no such kernel.
 * wpt_kernel_table_entry: row `index` of the table of the kernels the library has (WPT_ERR_INVALID_ARGUMENT behind its end). */
wpt_status wpt_kernel_choice(uint32_t need, uint32_t sensor, uint32_t count, uint32_t node_count, uint32_t tri_count, uint32_t material_count,
        uint32_t scene_has_wide, uint32_t variant, uint32_t walk, const char** name, const char** form, uint32_t key[4],
        uint64_t* scene_lds_bytes, uint32_t* materials_in_lds);
wpt_status wpt_kernel_table_entry(uint32_t index, uint32_t key[4], const char** name);
/* Which passes render a launch, from the facts the library decides by: a pure function that needs no device (tests; DESIGN.md
 * section 4 has the rule as a table).  sensor, count: as for wpt_kernel_choice; need: only its FEAT_RGL and FEAT_ANIM bits are
 * read; scene_in_lds: the launch's kernel keeps the scene in LDS (wpt_kernel_choice: scene_lds_bytes > 0); block_size: the
 * launch's pixels; samples_sqrt: 1 for an adaptive launch; cu_count: the device's compute units; variant, wavefront_mode,
 * slices: the words of wpt_set_launch_config, wpt_set_wavefront (mode) and wpt_set_slices.  plan: [WPT_PLAN_WAVEFRONT] 1: the
 * wavefront form renders the launch, and the words behind say how the single kernel does where [WPT_PLAN_WAVEFRONT_FALLS_BACK]
 * is 1 and the memory for the wavefront form cannot be had (0: a wavefront render reports every error); [WPT_PLAN_POOLED] the
 * pixels are handed out from the pixel pool; [WPT_PLAN_STRATEGY] one of WPT_STRATEGY_*; [WPT_PLAN_UNITS], [WPT_PLAN_ROWS] of a
 * sliced launch (else 1 and samples_sqrt); [WPT_PLAN_PASSES] what wpt_last_render_passes reports after the single kernel.
 * Where the memory a strategy needs cannot be had, the launch itself falls back to one pass; the plan does not say so. */
enum { WPT_PLAN_WAVEFRONT, WPT_PLAN_WAVEFRONT_FALLS_BACK, WPT_PLAN_POOLED, WPT_PLAN_STRATEGY, WPT_PLAN_UNITS, WPT_PLAN_ROWS, WPT_PLAN_PASSES,
    WPT_PLAN_WORDS };
enum { WPT_STRATEGY_ONE_PASS, WPT_STRATEGY_TWO_PASSES, WPT_STRATEGY_ADAPTIVE_ORDER, WPT_STRATEGY_SLICED };
wpt_status wpt_launch_plan(uint32_t sensor, uint32_t count, uint32_t need, uint32_t scene_in_lds, uint32_t block_size, uint32_t samples_sqrt,
        uint32_t cu_count, uint32_t variant, uint32_t wavefront_mode, uint32_t slices, uint32_t plan[WPT_PLAN_WORDS]);
/* What the reference records about a run for the CPU (wurblpt.hpp:393-400,425-435: COMPILER, CPU_MODEL), for the device:
 * marketing name and architecture of HIP device `device` ("AMD Instinct MI355X (gfx950:...)", or "" if there is none), and
 * the compiler and options the kernels were built with.  The strings live until the next call from the same thread. */
const char* wpt_device_name(int device);
/* Kernel launches the process's most recent render call took for its pixels: 1, or 2 when the frame was rendered in two
 * passes (timed first row of strata, then the rest with the longest tiles first), or the hundreds of trace + shade
 * launches of the wavefront form. Profilers see that many kernel launches per frame; what is rendered does not depend on it. */
uint32_t wpt_last_render_passes(void);
const char* wpt_build_info(void);

const char* wpt_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
