/*
 * rtmi.h — C-ABI of the MI355X-native (gfx950) trace/shade backend for
 * johnnovak/nim-raytracer.
 *
 * The reference has no FFI: its hot path is the Nim proc
 *     proc renderLine*(scene: Scene, opts: Options, fb: var Framebuf,
 *                      y: Natural, step: Natural = 1, maxStep: Natural = 1): Stats
 * (src/renderer/renderer.nim:162-211) plus proc initRenderer*()
 * (src/renderer/renderer.nim:214-215), called per scanline from worker
 * threads (src/raytracer.nim:25-32, src/concurrency/workerpool.nim:99).
 * This header is what a Nim `{.importc, dynlib: "librtmi.so".}` module binds
 * in its place. Plain C types only: pointers, sizes,
 * fixed-width integers and doubles. No torch/HIP types in any signature;
 * device streams are passed as opaque `void*` (a hipStream_t; NULL is HIP's
 * null stream, exactly as in the HIP API).
 *
 * Conventions
 *  - Every entry point returns int: RT_OK (0) or a negative RT_E_* code.
 *    The message of the last failure on the calling thread is available via
 *    rt_last_error(). No entry point aborts the caller's process.
 *  - Matrices are 4x4 column-major doubles exactly as glm stores Mat4x4
 *    (m[col*4 + row]); a point transforms as m * (x, y, z, 1).
 *  - The framebuffer is the reference's Framebuf layout
 *    (src/utils/framebuf.nim:7-28): w*h*3 float32, interleaved RGB,
 *    row-major, y = 0 is the top row. Caller-owned; the library never
 *    retains caller pointers after a call returns.
 */
#ifndef RTMI_H
#define RTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_ABI_VERSION 1

/* ---- error codes ------------------------------------------------------ */
enum {
  RT_OK = 0,
  RT_E_INVALID = -1,     /* bad argument (null pointer, size, index range) */
  RT_E_UNSUPPORTED = -2, /* valid request this build does not implement    */
  RT_E_DEVICE = -3,      /* HIP runtime / kernel failure, no usable GPU    */
  RT_E_NOMEM = -4,       /* host or device allocation failed               */
  RT_E_IO = -5           /* file could not be read / parsed                */
};

/* ---- scene description (flattened once from the Nim object graph) ----- */

/* Geometry kinds: Sphere / Plane / Box / TriangleMesh (src/renderer/geom.nim:137-155). */
enum rt_geom_type { RT_SPHERE = 0, RT_PLANE = 1, RT_BOX = 2, RT_MESH = 3 };

/* Light kinds: DistantLight / PointLight (src/renderer/light.nim:9-17). */
enum rt_light_type { RT_DISTANT_LIGHT = 0, RT_POINT_LIGHT = 1 };

/* AntialiasKind (src/renderer/renderer.nim:11-12). */
/* Antialias kinds (renderer.nim:14-21 AntialiasKind). The stochastic kinds
 * (sampling.nim:21-113) draw from a counter-based RNG keyed by
 * (rt_options.seed, absolute pixel, draw index) instead of the reference's
 * clock-seeded Nim `random` — reproducible, and independent of how rows are
 * split across calls, bands or GPUs. float32: (correlated) multi-jittered up
 * to grid_size 32; float64: up to 256. */
enum rt_aa_kind {
  RT_AA_NONE = 0,
  RT_AA_GRID = 1,
  RT_AA_JITTERED = 2,
  RT_AA_MULTI_JITTERED = 3,
  RT_AA_CORRELATED_MULTI_JITTERED = 4
};

/* Arithmetic precision of the device path. RT_FP64 repeats the reference's
 * float64 arithmetic operation for operation (parity mode); RT_FP32 is the
 * performance mode (parity within the tolerance stated in DESIGN.md). */
enum rt_precision { RT_FP32 = 0, RT_FP64 = 1 };

/* TriangleMesh data (src/renderer/geom.nim:151-155, src/loaders/obj.nim:87-126).
 * Face i uses vertices faces[3i..3i+2]; its normal is normals[3i..3i+2]
 * (one normal per face, obj.nim:65-84). normals == NULL means "compute as
 * obj.nim calcNormals does": normalize(cross(v1 - v0, v2 - v0)). */
typedef struct rt_mesh_desc {
  const double *vertices;  /* num_vertices * 3 (x, y, z), object space */
  int64_t num_vertices;
  const int32_t *faces;    /* num_faces * 3 zero-based vertex indices   */
  int64_t num_faces;
  const double *normals;   /* num_faces * 3, or NULL                    */
} rt_mesh_desc;

/* Object{geometry, material} (src/renderer/scene.nim:6-9,
 * src/renderer/material.nim:4-7). world_to_object is the caller's
 * objectToWorld.inverse (geom.nim:159-198), passed through unchanged so that
 * host and device use identical matrices. */
typedef struct rt_object_desc {
  int32_t type;                /* rt_geom_type                           */
  int32_t mesh;                /* RT_MESH: index into rt_scene_desc.meshes */
  double object_to_world[16];
  double world_to_object[16];
  double radius;               /* RT_SPHERE: Sphere.r                    */
  double box_min[3];           /* RT_BOX: aabb.vmin (object space)       */
  double box_max[3];           /* RT_BOX: aabb.vmax                      */
  double albedo[3];            /* Material.albedo                        */
  double reflection;           /* Material.reflection                    */
} rt_object_desc;

typedef struct rt_light_desc {
  int32_t type;                /* rt_light_type                          */
  int32_t reserved;
  double color[3];
  double intensity;
  double dir[3];               /* DistantLight.dir (travel direction)    */
  double pos[3];               /* PointLight.pos                         */
} rt_light_desc;

/* Mesh BVH builder. Either tree gives the brute-force answer (closest t,
 * lowest face index on ties), so images and Stats do not depend on it. */
typedef enum rt_bvh_builder {
  RT_BVH_SAH = 0,  /* host binned SAH (32 bins, leaves <= 4 faces): best tracing */
  RT_BVH_PLOC = 1  /* on the device: Morton sort + PLOC clustering + SAH leaf
                      collapse, same node format; ~100x faster to build. A
                      mesh whose clustered tree is deeper than the kernels'
                      traversal stack (60; boxes nested around one corner,
                      such as a fan of geometrically growing faces) is built
                      by the host builder instead: a mesh RT_BVH_SAH accepts
                      is never refused here                                  */
} rt_bvh_builder;

/* Scene (src/renderer/scene.nim:11-18). */
typedef struct rt_scene_desc {
  const rt_object_desc *objects;
  int32_t num_objects;
  int32_t num_lights;
  const rt_light_desc *lights;
  const rt_mesh_desc *meshes;
  int32_t num_meshes;
  int32_t bvh_builder;         /* rt_bvh_builder (0 = host binned SAH)    */
  double fov;                  /* degrees, Scene.fov                     */
  double camera_to_world[16];  /* Scene.cameraToWorld                    */
  double bg_color[3];          /* Scene.bgColor                          */
} rt_scene_desc;

/* Options (src/renderer/renderer.nim:24-28) plus the device-path knobs. */
typedef struct rt_options {
  int32_t width, height;       /* Options.width/height                   */
  int32_t aa_kind;             /* Options.antialias.kind (rt_aa_kind)    */
  int32_t grid_size;           /* Options.antialias.gridSize (m)         */
  double bias;                 /* Options.bias                           */
  int32_t max_ray_depth;       /* Options.maxRayDepth                    */
  int32_t precision;           /* rt_precision                           */
  uint64_t seed;               /* stochastic samplers: counter-RNG seed  */
  uint32_t flags;              /* RT_FLAG_*                              */
  uint32_t reserved;
} rt_options;

/* Accepted for compatibility and ignored: shadow rays always stop searching
 * a mesh once the reference's outcome and hit count are decided (an exact
 * early exit: image and Stats identical to the closest-hit reference). */
#define RT_FLAG_ANYHIT_SHADOWS 0x1u
/* Run the instrumented kernel that also counts BVH node / triangle record
 * fetches (rt_scene_last_counters). Slower; the image and Stats are the same. */
#define RT_FLAG_COUNT_TRAVERSAL 0x2u
/* float32 kernel: always hand pixel groups out in screen order. By default a
 * short launch (a band set of a multi-GPU frame) that repeats a mapping already
 * rendered on this scene hands them out longest-first, from per-group
 * durations measured on its first launch. Scheduling only: the image and
 * Stats are the same either way. */
#define RT_FLAG_NO_REORDER 0x4u
/* float32 kernel: search the mesh BVH for every ray. By default camera rays
 * (>= 16 samples per pixel) and shadow rays to distant lights of a scene with
 * one mesh object search the faces binned for their pixel / light-grid cell
 * instead. The image and Stats are the same either way. */
#define RT_FLAG_NO_BINNING 0x8u
/* float32 kernel: render every pixel group with the one general kernel. By
 * default a launch whose pixel records mark pixels lean (no camera ray can hit
 * the scene's mesh and every light is a distant light whose shadow rays
 * provably miss it) renders those pixels with a second, lean-only kernel from
 * a per-launch list. Scheduling only: the image and Stats are the same. */
#define RT_FLAG_NO_SPLIT 0x10u
/* float32 kernel, two-class launches: render the general (not lean) pixels
 * with the one-sample loop of the general kernel. By default, in scenes of
 * one mesh object with distant lights only and no reflection, they render in
 * a kernel that carries several samples per lane through each face list
 * (falling back to the one-sample loop for a pixel whose shadow rays need
 * the BVH). Scheduling only: the image and Stats are the same. */
#define RT_FLAG_NO_BATCH 0x20u
/* Test hook: the batched general kernel discards each general pixel's
 * batches at its last one and re-renders the pixel with the one-sample loop
 * (the path it takes when a shadow ray needs the BVH). Same image and Stats. */
#define RT_FLAG_BATCH_FALLBACK 0x40u
/* float32 kernel, two-class launches: render lean pixels with the general
 * lean kernel. By default, in scenes whose only analytic object is one
 * translated plane (a mesh on a ground plane) with one or two distant lights
 * and akGrid sampling of m | 64 with spp a multiple of 256, they render in a
 * kernel specialised for that case. Scheduling only: same image and Stats. */
#define RT_FLAG_NO_LEAN1 0x80u
/* float32 kernel, two-class launches in the same one-plane scenes: render the
 * general pixels with the general batched kernel instead of the one
 * specialised for them. Scheduling only: same image and Stats. */
#define RT_FLAG_NO_GEN1 0x100u
/* _device calls with out == NULL: the caller will not read this call's Stats
 * (rt_scene_last_stats then fails), so the per-call Stats reduction is not
 * launched — the render kernels are all the call puts on the stream. Ignored
 * when out != NULL or with RT_FLAG_COUNT_TRAVERSAL. */
#define RT_FLAG_NO_STATS 0x200u
/* float32 kernel, one-plane two-class launches: launch the general and the
 * lean pixels' kernels separately. By default both lists run in one merged
 * kernel (general items first, then lean ones). Same image and Stats. */
#define RT_FLAG_NO_MIX 0x400u
/* Record HIP events (on the call's stream) around the call's two parts: the
 * camera-dependent data it builds on the device (camera-ray face lists, pixel
 * records, lean / general lists, object masks) and its render kernels;
 * rt_scene_last_timing reads them. Same image and Stats. */
#define RT_FLAG_TIMING 0x800u
/* float32 kernel, scenes of spheres / boxes / planes with distant lights and
 * no reflection: trace one sample per lane at a time. By default such pixels
 * carry 4 samples per lane through their object-binned object and light
 * loops (and a 64-spp frame uses 16 lanes per pixel to fill that batch).
 * Same image and Stats. */
#define RT_FLAG_NO_OBJ_BATCH 0x1000u
/* float32 kernel, scenes with reflective materials: queue the reflected rays
 * per wave and trace them in full 64-ray passes (k_render_wave), the pixel's
 * deeper levels summed in 32.32 fixed point — the image differs from the
 * default by float rounding only, the Stats are the same. By default each
 * reflected ray is traced in the lane of its camera sample, one level after
 * another: measured faster on the scenes here, whose reflected rays stay
 * coherent within a wave (DESIGN.md "Reflection-ray compaction"). */
#define RT_FLAG_COMPACT 0x2000u
/* float64 (parity) mode: render with one lane per pixel and the BVH for every
 * ray the pixel records do not rule out. By default akGrid frames of >= 64
 * samples per pixel render one pixel per wave (64 samples side by side; the
 * camera rays search the pixel's face list and the shadow rays to distant
 * lights their light-grid cells), each pixel's samples still summed in sample
 * order. The image and Stats are the same, bit for bit. */
#define RT_FLAG_F64_PER_LANE 0x4000u
/* One-plane two-class launches: do not classify the lean pixels. By default
 * the per-call build proves, in the float32 arithmetic of the lean kernel,
 * which lean pixels have samples that all hit the plane unshadowed or all
 * miss it; the kernel writes such a pixel's fixed sum of one constant without
 * running its sample loop. The image and Stats are the same, bit for bit
 * (tests/test_gpu_uniform.py). */
#define RT_FLAG_NO_UNIFORM 0x8000u
/* One-plane two-class launches: do not tag ground pixels. By default the
 * per-call build tags the general pixels that have an empty camera-ray list
 * and pass the uniform-lit proof above (flat ground in the mesh's shadow):
 * every sample hits the plane and only its shadow rays can meet the mesh, so
 * the batched kernel gives them a sample loop of their own (the shadow
 * searches alone). The image and Stats are the same, bit for bit
 * (tests/test_gpu_ground.py). */
#define RT_FLAG_NO_GROUND1 0x10000u
/* One-plane launches with the one-plane batched kernel: no shortcuts for the
 * mesh pixels (general pixels with a camera-ray list). By default a sample
 * slot whose lit shadow origins all lie strictly inside the mesh's box, inset
 * by the call's margin, skips the mesh's box gate of every light (the gate is
 * proved false there), and a batch whose samples all hit the mesh, every one
 * of them inside, is shaded on a straight path without the hit-kind selects.
 * The image and Stats are the same, bit for bit (tests/test_gpu_mesh1.py). */
#define RT_FLAG_NO_MESH1 0x20000u

/* Stats (src/renderer/stats.nim:4-13) plus ray counts for Mray/s. */
typedef struct rt_stats {
  uint64_t num_primary_rays;        /* renderer.nim:138,155             */
  uint64_t num_intersection_tests;  /* renderer.nim:58                  */
  uint64_t num_intersection_hits;   /* renderer.nim:65                  */
  uint64_t num_shadow_rays;         /* one per light per shaded hit     */
  uint64_t num_reflection_rays;     /* renderer.nim:114-118             */
} rt_stats;

/* Device-side work counters of the last render (algorithmic traffic). */
typedef struct rt_traversal_counters {
  uint64_t wave_node_fetches;  /* BVH node records fetched (per wave)     */
  uint64_t wave_tri_fetches;   /* triangle records fetched (per wave)     */
  uint64_t lane_node_visits;   /* sum over rays of node records visited
                                  (a ray visits a node whose box it hit)  */
  uint64_t lane_tri_tests;     /* sum over rays of triangle tests         */
} rt_traversal_counters;

typedef struct rt_scene_info {
  int64_t num_objects, num_lights, num_meshes;
  int64_t num_triangles;       /* all meshes                             */
  int64_t num_bvh_nodes;       /* all meshes                             */
  int32_t max_bvh_depth;
  int32_t device;
  int64_t device_bytes;        /* scene bytes in HBM: geometry, BVH, bins and the per-call buffer sets */
  double build_ms;             /* host BVH build + upload wall time      */
} rt_scene_info;

typedef struct rt_scene rt_scene; /* opaque, owns device buffers */

/* ---- library ----------------------------------------------------------- */

/* ABI version of the loaded library (RTMI_ABI_VERSION). */
int rt_version(void);

/* Hash of the native sources the library was built from (16 hex digits:
 * sha256 of csrc/, the Makefile and this header, nim-raytracer_amd/rtmi/
 * srchash.py): build provenance for benchmarks and profiles. */
const char *rt_build_source_hash(void);

/* Message of the last failed call on this thread ("" if none). */
const char *rt_last_error(void);

/* initRenderer* (renderer.nim:214-215) equivalent: bind the calling thread
 * to HIP device `device` and check it is a gfx950 GPU. Safe to call again. */
int rt_init(int device);

/* Number of visible GPUs (0 when none; never fails). */
int rt_device_count(void);

/* ---- scene ------------------------------------------------------------- */

/* Flatten, build the per-mesh BVH and upload everything to the current
 * device. desc and all arrays it points to may be freed after return.
 * RT_E_INVALID, under either builder, for a non-finite vertex that a face
 * references (as rt_scene_set_mesh_vertices). */
int rt_scene_create(const rt_scene_desc *desc, rt_scene **out_scene);
/* Waits for a call still running on the scene in another thread, then frees
 * it. No call may START on a scene once its destroy has begun (the caller's
 * own bookkeeping: INTEGRATION.md's binding retires a replaced scene only
 * after its in-flight renderLine calls have returned). */
int rt_scene_destroy(rt_scene *scene);
int rt_scene_get_info(const rt_scene *scene, rt_scene_info *out);

/* Replace the scene's camera: Scene.cameraToWorld (column-major, glm) and
 * Scene.fov in degrees (scene.nim:14-16), which renderLine re-reads on every
 * call (renderer.nim:135-136, 150-153 via castPrimaryRay :31-44). Takes
 * effect from the next render call; the geometry, BVH and light grids are
 * kept (every camera-dependent structure is rebuilt by each render call
 * anyway). Waits for the scene's earlier calls. RT_E_INVALID for a non-finite
 * matrix or a fov outside (0, 180). */
int rt_scene_set_camera(rt_scene *scene, const double camera_to_world[16],
                        double fov_deg);

/* Replace the scene's lights (Scene.lights, scene.nim). From the next call on
 * the scene behaves exactly as one created by rt_scene_create from the same
 * description with these lights: frames in both precisions, Stats, the
 * rt_scene_last_* diagnostics and which kernels run are the same, bit for bit.
 * Any count >= 0 and any mix of light types; the count and types may differ
 * from the current ones. Geometry, BVH, triangle records, camera and buffer
 * sets are kept; the distant lights' mesh grids are rebuilt on the device from
 * the resident faces. Waits for the scene's earlier calls (renders, pipelined
 * builds, queries). RT_E_INVALID for a negative count, a null array with a
 * non-zero count or a bad light type. On any failure the scene keeps its
 * previous lights. */
int rt_scene_set_lights(rt_scene *scene, const rt_light_desc *lights,
                        int32_t num_lights);

/* Replace the vertex positions of mesh `mesh` (index into the rt_scene_desc.meshes
 * the scene was created from). The face index array, the vertex count and the
 * face count stay: num_vertices must equal the count given at create. normals:
 * num_faces*3 face normals, or NULL = recompute as rt_scene_create does for
 * rt_mesh_desc.normals == NULL (calcNormals).
 * From the next call on the scene answers exactly as one created by
 * rt_scene_create from the same description with these vertices: frames in
 * both precisions, Stats, the rt_trace_rays / rt_pick_pixels answers (t, obj,
 * face, normals), rt_scene_last_split and rt_scene_last_lean_kernel are the
 * same, bit for bit. The tree keeps the topology and leaf order it was built
 * with; only its boxes are refitted (on the device), so traversal may be
 * slower than on a fresh tree after a large deformation, never different.
 * Waits for everything in flight on the scene (renders, pipelined builds,
 * queries). Camera, lights, objects, materials, buffer sets and the other
 * meshes are kept; the light grids are rebuilt over the new faces.
 * RT_E_INVALID for a null scene or vertex array, a mesh index out of range,
 * a num_vertices different from the mesh's, or a non-finite vertex that a
 * face references. On any failure the scene keeps its previous geometry.
 * A mesh of 0 faces is RT_OK and launches nothing. */
int rt_scene_set_mesh_vertices(rt_scene *scene, int32_t mesh, const double *vertices,
                               int64_t num_vertices, const double *normals);
/* The same with the arrays in device memory (a deformation computed on the GPU:
 * nothing crosses PCIe). The arrays are read after the work already enqueued on
 * hip_stream; the call returns when the scene is updated and the buffers may be
 * reused. */
int rt_scene_set_mesh_vertices_device(rt_scene *scene, int32_t mesh, const double *d_vertices,
                                      int64_t num_vertices, const double *d_normals,
                                      void *hip_stream);

/* Replace every object's transform pair, radius, box_min / box_max, albedo and
 * reflection (Scene.objects' geometry placement and Material): move and
 * restyle objects in place. num_objects must equal the scene's object count,
 * each object's type the one given at create and, for RT_MESH, its mesh the
 * one given at create: RT_E_INVALID otherwise, with the object's index in the
 * message. Matrices are checked as rt_scene_create checks them (non-affine:
 * RT_E_UNSUPPORTED).
 * From the next call on the scene answers exactly as one created by
 * rt_scene_create from the same description with these objects: frames in
 * both precisions, Stats, the rt_trace_rays / rt_pick_pixels answers, the
 * rt_scene_last_* diagnostics and which kernels run are the same, bit for bit.
 * The meshes (with the vertices of any mesh update), both trees, the triangle
 * records, normals, lights' descriptions, camera and buffer sets are kept;
 * the object records, the objects' world boxes and everything that depends on
 * both the lights and the objects (the light grids over the one mesh object,
 * the object light grids of 4..64-object scenes, both built on the device)
 * are formed again. Waits for everything in flight on the scene. On any
 * failure the scene keeps its previous objects. */
int rt_scene_set_objects(rt_scene *scene, const rt_object_desc *objects,
                         int32_t num_objects);

/* ---- rendering ----------------------------------------------------------
 * All render calls implement renderLine (renderer.nim:162-211) for every row
 * y in countup(y0, y1 - 1, step):
 *   for x in countup(0, width - 1, step):
 *     if step < maxStep and (x and (2*step-1)) == 0 and (y and (2*step-1)) == 0:
 *       continue                      # already rendered at a coarser level
 *     color = calcPixel(...)          # akNone: 1 sample at (x, y); akGrid: m*m
 *     fill fb[x..x+step-1, y..y+step-1] (clipped) with color
 * step and max_step must be powers of two with max_step >= step.
 * `out` receives the summed Stats of the call (may be NULL for the _device
 * forms, which then do not synchronise the stream).
 * The per-call camera-dependent build has no capacity failure: a pixel
 * whose face list outgrows its slots keeps its true length and its camera
 * rays take the BVH (the same answers).
 */

/* Host framebuffer form: fb_rgb is caller memory of fb_w*fb_h*3 floats with
 * fb_w == opts->width and fb_h == opts->height. Thread-safe: concurrent
 * callers on disjoint rows are serialised internally (renderLine is called
 * concurrently by the reference's pool, workerpool.nim:172-223). */
int rt_render_lines(rt_scene *scene, const rt_options *opts, float *fb_rgb,
                    int32_t fb_w, int32_t fb_h, int32_t y0, int32_t y1,
                    int32_t step, int32_t max_step, rt_stats *out);

/* Device framebuffer form (the fast path: whole frame, nothing crosses
 * PCIe). d_fb is a device pointer to width*height*3 floats. */
int rt_render_lines_device(rt_scene *scene, const rt_options *opts,
                           float *d_fb, int32_t y0, int32_t y1, int32_t step,
                           int32_t max_step, void *hip_stream, rt_stats *out);

/* Multi-GPU shard: image rows are cut into bands of band_h rows; band b is
 * owned by rank b % world. Renders this rank's bands (step 1) into the
 * compact device buffer d_bands laid out as
 *   [ceil(ceil(height/band_h)/world) * band_h rows][width][3] float32,
 * i.e. local band k occupies rows [k*band_h, (k+1)*band_h). Rows past the
 * image bottom are left untouched. */
int rt_render_bands_device(rt_scene *scene, const rt_options *opts,
                           float *d_bands, int32_t band_h, int32_t rank,
                           int32_t world, void *hip_stream, rt_stats *out);

/* Rank-0 epilogue of the framebuffer gather: d_gathered holds `world`
 * compact band buffers back to back (an all-gather of rt_render_bands_device
 * outputs); writes the interleaved image to d_fb (width*height*3). */
int rt_unshard_bands_device(const float *d_gathered, float *d_fb,
                            int32_t width, int32_t height, int32_t band_h,
                            int32_t world, void *hip_stream);

/* Rows per rank-local compact band buffer (helper for sizing d_bands). */
int rt_band_rows(int32_t height, int32_t band_h, int32_t world,
                 int32_t *out_rows);

/* Stats of the last render call on this scene (waits for it): for
 * asynchronous _device calls made with out == NULL (RT_E_INVALID if that
 * call set RT_FLAG_NO_STATS). */
int rt_scene_last_stats(rt_scene *scene, rt_stats *out);

/* Durations of the last call made with RT_FLAG_TIMING (waits for it): its
 * per-call camera-dependent build and its render kernels (incl. the Stats
 * reduction), in milliseconds. RT_E_INVALID if that call did not set the flag. */
int rt_scene_last_timing(rt_scene *scene, double *setup_ms, double *render_ms);

/* ---- one process, several GPUs (SURVEY.md 8(b) rt_render_frame_multi) ---- */

/* The scene replicated on every listed device (a device may repeat: several
 * ranks on one GPU); rows cut into band_h-row bands dealt round-robin
 * (band b -> rank b % num_devices; band_h 0 means 4); every rank renders its
 * bands on its own device at the same time, the compact band buffers move to
 * devices[0] over xGMI (peer copies) and are un-interleaved there. Images and
 * Stats equal the single-device frame. For one process per GPU use
 * rt_render_bands_device + rt_unshard_bands_device with RCCL instead. */
typedef struct rt_multi rt_multi;
int rt_multi_create(const rt_scene_desc *desc, const int32_t *devices,
                    int32_t num_devices, int32_t band_h, rt_multi **out);
/* Whole frame (step 1) into d_fb, a width*height*3 float32 buffer on
 * devices[0]; out != NULL waits for the frame and sums the Stats. */
int rt_render_frame_multi_device(rt_multi *m, const rt_options *opts,
                                 float *d_fb, rt_stats *out);
/* Whole frame into the caller's host framebuffer (fb_w*fb_h*3 floats). */
int rt_render_frame_multi(rt_multi *m, const rt_options *opts, float *fb,
                          int32_t fb_w, int32_t fb_h, rt_stats *out);
/* rt_scene_set_camera on every rank's scene. */
int rt_multi_set_camera(rt_multi *m, const double camera_to_world[16],
                        double fov_deg);
/* rt_scene_set_lights on every rank's scene. */
int rt_multi_set_lights(rt_multi *m, const rt_light_desc *lights,
                        int32_t num_lights);
/* rt_scene_set_mesh_vertices on every rank's scene. */
int rt_multi_set_mesh_vertices(rt_multi *m, int32_t mesh, const double *vertices,
                               int64_t num_vertices, const double *normals);
/* rt_scene_set_objects on every rank's scene. */
int rt_multi_set_objects(rt_multi *m, const rt_object_desc *objects,
                         int32_t num_objects);
int rt_multi_destroy(rt_multi *m);

/* ---- render queue (workerpool.nim WorkerPool[WorkMsg, ResponseMsg]) ---- */

/* The pool raytracer.nim and gui.nim drive (src/concurrency/workerpool.nim;
 * WorkMsg / ResponseMsg, src/raytracer.nim:13-32; gui.nim:98-122,206-280),
 * over the GPU: one host thread per queue takes the longest run of queued
 * lines that share options, framebuffer, step and max_step and follow each
 * other at `step`, and renders it with ONE rt_render_lines call (one launch
 * per refinement level when the caller queues a whole level, as gui.nim
 * does). Every message gets its own response, in queue order; a run's Stats
 * ride on its last line's response, the others carry zero Stats (callers sum
 * them). States and return values follow workerpool.nim; every command has
 * completed when it returns, so the queue is always ready (isReady). The
 * queue must be destroyed before its scene. */
typedef struct rt_queue rt_queue;

typedef enum rt_queue_state_kind {
  RT_QUEUE_STOPPED = 0, /* wsStopped: work is queued, not started */
  RT_QUEUE_RUNNING = 1, /* wsRunning                             */
  RT_QUEUE_SHUTDOWN = 2 /* wsShutdown: no more work accepted       */
} rt_queue_state_kind;

typedef struct rt_response { /* ResponseMsg (raytracer.nim:21-23) + the line */
  int32_t line;
  int32_t status;            /* RT_OK, or the render call's error code    */
  rt_stats stats;
  char error[128];           /* rt_last_error() text when status != 0     */
} rt_response;

/* initRenderWorkers (raytracer.nim:35-38); starts stopped. */
int rt_queue_create(rt_scene *scene, rt_queue **out);
/* start / stop (workerpool.nim:253-275): 1 done, 0 not in the required
 * state (stopped / running). stop lets the batch in flight finish and
 * keeps queued lines queued. */
int rt_queue_start(rt_queue *q);
int rt_queue_stop(rt_queue *q);
int rt_queue_state(rt_queue *q);    /* rt_queue_state_kind, or < 0 */
int rt_queue_is_ready(rt_queue *q); /* 1 */
/* queueWork (workerpool.nim:235): renderLine(line, step, maxStep) into the
 * caller's host framebuffer fb (fb_w*fb_h*3 floats, written by the queue's
 * thread until the line's response arrives); step / max_step 0 mean 1
 * (raytracer.nim:26-27). */
int rt_queue_work(rt_queue *q, const rt_options *opts, float *fb,
                  int32_t fb_w, int32_t fb_h, int32_t line, int32_t step,
                  int32_t max_step);
/* tryRecvResult (workerpool.nim:240): 1 and *out filled, or 0 if no
 * response is waiting. A failed line's message is also set as this
 * thread's rt_last_error(). */
int rt_queue_try_recv(rt_queue *q, rt_response *out);
/* Lines queued or in flight. */
int rt_queue_pending(rt_queue *q);
/* reset (workerpool.nim:285-314): stop, drop queued work and undelivered
 * responses; 1 done, 0 after shutdown. */
int rt_queue_reset(rt_queue *q);
/* shutdown (workerpool.nim:359): 1 done, 0 if already shut down. */
int rt_queue_shutdown(rt_queue *q);
/* close (workerpool.nim:371) + free, from any state. */
int rt_queue_destroy(rt_queue *q);

/* ---- output (framebuf.nim:55-93 writePpm) ------------------------------ */

/* The P6 payload of writePpm for a device framebuffer (width*height*3
 * float32, the Framebuf.data layout): per component clamp to [0, 1], optional
 * linearToSRGB (color.nim:17-22), round(c * (2^bits - 1)); bits in 1..16;
 * bits <= 8: one byte per component, else two bytes big-endian. d_out
 * receives rt_ppm_payload_bytes() bytes (device memory). Replaces
 * framebuf.nim:82-88's per-component loop; the caller writes
 * rt_ppm_header() and then the payload. */
int rt_ppm_encode_device(const float *d_fb, int32_t width, int32_t height,
                         int32_t bits, int32_t srgb, void *d_out,
                         void *hip_stream);
/* Payload size in bytes (width*height*3*(bits <= 8 ? 1 : 2)), or < 0. */
int64_t rt_ppm_payload_bytes(int32_t width, int32_t height, int32_t bits);
/* writeHeader (framebuf.nim:60-61): "P6 <w> <h> <maxval> " into buf; returns
 * its length (excluding the NUL), or < 0 if buf_len is too small. */
int rt_ppm_header(int32_t width, int32_t height, int32_t bits, char *buf,
                  int32_t buf_len);

/* ImageRGBA.copyFrom (src/utils/image.nim:45-54) as a GPU post-pass: the
 * width*height*3 float32 device framebuffer -> width*height RGBA8 pixels at
 * d_out (device memory, 4-B aligned), round(c * 0xff).uint8 per component
 * and `alpha`, for the GUI's texture upload without a float32 round trip.
 * No clamp, like the reference: components outside [0, 255] after rounding
 * keep the low 8 bits of the x86-64 int32 conversion (the reference's
 * release build). Asynchronous on `stream`. */
int rt_rgba_encode_device(const float *d_fb, int32_t width, int32_t height,
                          uint8_t alpha, void *d_out, void *stream);

/* Traversal counters of the last render call on this scene (waits for it).
 * Zero unless that call set RT_FLAG_COUNT_TRAVERSAL. */
int rt_scene_last_counters(rt_scene *scene, rt_traversal_counters *out);

/* Work split of the last render call on this scene: pixel groups rendered by
 * the lean-pixel kernel and by the general kernel (RT_FLAG_NO_SPLIT; a
 * float64 call counts every group as general). Host-side bookkeeping, no wait. */
int rt_scene_last_split(rt_scene *scene, int64_t *lean_groups, int64_t *general_groups);
/* Of the last render call's general pixel groups: how many went to the
 * batched general kernel (0 with RT_FLAG_NO_BATCH or where it does not
 * apply), and how many of those it re-rendered with the one-sample loop
 * because a shadow ray needed the BVH (as of the last call that returned
 * Stats; -1 before any). Diagnostics for tests and the benchmark. */
int rt_scene_last_batch(rt_scene *scene, int64_t *batched_groups, int64_t *fallback_groups);
/* Which kernels rendered the last call's two classes: bits 0-1 the lean
 * pixels' (0 none — no two-class launch, 1 the general lean kernel, 2 the
 * one-plane lean kernel, RT_FLAG_NO_LEAN1), bits 2-3 the general pixels'
 * (0 the one-sample kernel, 1 the general batched kernel, 2 the one-plane
 * batched kernel, RT_FLAG_NO_GEN1); 3 in both: the merged one-plane kernel
 * (RT_FLAG_NO_MIX); bit 4: reflected rays compacted per wave (reflective
 * scenes, RT_FLAG_COMPACT); bits 8-15: lanes per lean pixel of a two-class
 * call (4 or 16 for the one-plane lean kernel, kind 2 or 3; 64, one pixel
 * per wave, only with the general lean kernel, kind 1; 0 otherwise) — mask with 0x1f to compare the kernel kinds. Host-side
 * bookkeeping, no wait. */
int rt_scene_last_lean_kernel(rt_scene *scene, int32_t *kind);
/* Of the last render call's lean pixel groups (rt_scene_last_split counts
 * them all): how many the per-call build proved uniform-lit and uniform-sky,
 * so that the lean kernel skipped their sample loops. Both 0 when the call
 * classified nothing (RT_FLAG_NO_UNIFORM, not a one-plane two-class launch).
 * Waits for the call. */
int rt_scene_last_uniform(rt_scene *scene, int32_t *lit, int32_t *sky);
/* Of the last render call's general pixel groups (rt_scene_last_split and
 * rt_scene_last_batch count them all): how many the per-call build tagged as
 * ground pixels. 0 when the call tagged nothing (RT_FLAG_NO_GROUND1, not a
 * one-plane two-class launch with the one-plane batched kernel). Waits for
 * the call. */
int rt_scene_last_ground(rt_scene *scene, int32_t *ground);
/* Of the last render call's batches of mesh-pixel samples (64 lanes x the
 * batch's samples per lane, in the one-plane batched kernel): how many took
 * the straight path of the description of RT_FLAG_NO_MESH1. 0 with that flag,
 * for a call the one-plane batched kernel did not serve, and for a call that
 * counted traversal steps. Valid once the call's Stats have been read (a
 * render call given `stats`, or rt_scene_last_stats); RT_E_INVALID after a
 * call that set RT_FLAG_NO_STATS. */
int rt_scene_last_mesh1(rt_scene *scene, int64_t *straight_batches);

/* ---- ray queries --------------------------------------------------------
 * trace (renderer.nim:47-67) itself — "what does this ray hit, and where" —
 * for batches of caller-supplied rays and for picks through the camera:
 * what a GUI needs for the object under the mouse, a tool to place something
 * on a surface, a line-of-sight test. float64 only: the answers are the
 * reference's, operation for operation (the float32 mode's hits:
 * rt_trace_rays_f32 and rt_pick_pixels_f32 below).
 *
 * Ray i is the world-space (orig[3i..3i+2], 1), (dir[3i..3i+2], 0) of initRay
 * (geom.nim:41-48); dir is taken as given, NOT normalised, so t is in units
 * of |dir|. The answer is trace(ray, scene.objects, tNear): the closest t
 * with 0 <= t < t_near, the first object in scene order on equal t, the
 * lowest face index on equal t within a mesh — including
 * TriangleMesh.intersect's AABB gate (geom.nim:339-358): a ray that starts
 * inside a mesh's box misses that mesh. t_near == NULL means +inf for every
 * ray.
 *  - Miss: obj = -1, face = -1, t = that ray's t_near.
 *  - RT_QUERY_ANY_HIT: trace as shade calls it for shadow rays (renderer.nim:
 *    96-99), with their exact early exit: only obj >= 0 versus obj == -1 is
 *    meaningful. t and face are not computed (t echoes t_near, face is -1).
 *    The Stats are still the reference's.
 *  - A degenerate ray — a non-finite component, an all-zero direction or a
 *    NaN t_near — is answered as a miss with its t_near as given and adds
 *    nothing to the Stats.
 *  - normals (may be NULL) receives per ray the vector shade calls hitNormal
 *    (renderer.nim:83-88): objectToWorld * normal(hitO) for spheres, planes
 *    and boxes, objectToWorld * normals[face] for mesh hits; xyz, not
 *    renormalised; (0, 0, 0) on a miss. RT_E_INVALID with RT_QUERY_ANY_HIT.
 *  - out (may be NULL) receives num_intersection_tests and
 *    num_intersection_hits as renderer.nim:58,65 count them over the batch,
 *    the other fields 0 (picks: num_primary_rays, see rt_pick_pixels).
 *    A _device call with out == NULL only enqueues work on hip_stream; with
 *    out it waits for the answers.
 *  - RT_QUERY_SORT: the rays are traced in the order of a 32-bit coherence
 *    key formed on the device (direction octant, then a Morton code of the
 *    origin within the batch's origin bounds, or of the direction when every
 *    ray shares one origin; picks: a Morton code of the pixel position), the
 *    answers written back in input order: hits, normals and Stats are the
 *    same, byte for byte. Whether it is faster depends on the batch
 *    (DESIGN.md "Ray queries"); off by default.
 * Queries take the scene's lock, are ordered after a render still in flight
 * on the scene, and leave what rt_scene_last_stats, _last_split, _last_batch,
 * _last_lean_kernel, _last_uniform, _last_ground, _last_timing and
 * _last_counters report untouched: those stay the last render call's.
 * n == 0 is RT_OK and launches nothing; n < 0, unknown flag bits and null
 * required pointers are RT_E_INVALID; n >= 2^31 is RT_E_UNSUPPORTED. */
typedef struct rt_hit {     /* 16 bytes */
  double  t;                /* tHit; on a miss: that ray's t_near          */
  int32_t obj;              /* index into rt_scene_desc.objects, -1 = nil  */
  int32_t face;             /* original face index of a mesh hit, else -1  */
} rt_hit;

#define RT_QUERY_ANY_HIT 0x1u  /* shadow-ray semantics */
#define RT_QUERY_SORT    0x2u  /* reorder rays for coherence before tracing */

/* Device form: d_orig / d_dir (n*3 doubles), d_tnear (n doubles or NULL),
 * d_hits (n rt_hit) and d_normals (n*3 doubles or NULL) are device memory. */
int rt_trace_rays_device(rt_scene *scene, int64_t n, const double *d_orig,
                         const double *d_dir, const double *d_tnear,
                         uint32_t flags, rt_hit *d_hits, double *d_normals,
                         void *hip_stream, rt_stats *out);
/* Host form: the same arrays in caller memory; returns with the answers. */
int rt_trace_rays(rt_scene *scene, int64_t n, const double *orig,
                  const double *dir, const double *tnear, uint32_t flags,
                  rt_hit *hits, double *normals, rt_stats *out);

/* Picking: ray i is castPrimaryRay(opts->width, opts->height, xy[2i],
 * xy[2i+1], fov, cameraToWorld) (renderer.nim:31-44) with the scene's current
 * camera (rt_scene_set_camera applies), formed on the device exactly as the
 * float64 render forms it, and traced with t_near = +inf. Integer (x, y) is
 * the akNone sample of that pixel; fractional coordinates and coordinates
 * outside the image are legal; a non-finite coordinate makes the ray
 * degenerate. Only width, height and precision of opts are read; precision
 * must be RT_FP64 (RT_FP32 is RT_E_UNSUPPORTED here: rt_pick_pixels_f32 is
 * the float32 render's pick). flags, hits, normals and out
 * as above; out->num_primary_rays is the number of rays that are not
 * degenerate. */
int rt_pick_pixels_device(rt_scene *scene, const rt_options *opts, int64_t n,
                          const double *d_xy, uint32_t flags, rt_hit *d_hits,
                          double *d_normals, void *hip_stream, rt_stats *out);
int rt_pick_pixels(rt_scene *scene, const rt_options *opts, int64_t n,
                   const double *xy, uint32_t flags, rt_hit *hits,
                   double *normals, rt_stats *out);

/* ---- radiance queries ---------------------------------------------------
 * shade (renderer.nim:71-127) itself — "what colour does this ray see" — for
 * batches of caller-supplied rays: an orthographic, panoramic, stereo or
 * thin-lens camera with its own samples, a light probe or cube map at a
 * point, radiance baked at surface points, a preview of what a mirror shows.
 * The caller forms the rays; the library answers with the reference's colour,
 * float64 operation for operation (the float32 mode's colours:
 * rt_shade_rays_f32 below).
 *
 * Ray i is initRay(orig_i, dir_i) (geom.nim:41-48) with depth 1; dir is taken
 * as given, NOT normalised, as in rt_trace_rays. Its colour is
 * shade(ray, trace(ray, scene.objects, +inf)) (renderer.nim:47-127): hitNormal,
 * getShadingInfo, one shadow ray per light, shadeDiffuse and the reflection
 * recursion — what calcPixelNoSampling computes once castPrimaryRay has
 * formed the ray. A miss gives bgColor. The scene's camera is not read.
 *  - opts: only bias, max_ray_depth and precision are read (width, height
 *    and antialias are ignored). precision must be RT_FP64 (RT_FP32 is
 *    RT_E_UNSUPPORTED); with reflective materials max_ray_depth above 7 is
 *    RT_E_UNSUPPORTED, as for a render.
 *  - group >= 1 and n % group == 0, else RT_E_INVALID; the outputs hold
 *    n / group colours. group == 1: output i is ray i's colour as computed
 *    (no sum and no multiply: a -0.0 stays -0.0). group > 1: output k is
 *    calcPixel's expression (renderer.nim:147-159) over rays k*group ..
 *    k*group + group - 1: from vec3(0), the colours added in index order,
 *    then one multiplication by 1.0 / group.
 *  - rgb: float64, three per colour. rgb32: the same values converted to
 *    float32 as Framebuf stores them, so a custom-camera image can go
 *    straight to rt_ppm_encode_device / rt_rgba_encode_device. Either may be
 *    NULL; both NULL with n > 0 is RT_E_INVALID.
 *  - A degenerate ray — a non-finite component or an all-zero direction —
 *    has the colour (0, 0, 0) and adds nothing to the Stats; it contributes
 *    +0 to its group's sum, and the group still divides by `group`.
 *  - out (may be NULL) receives all five fields: num_primary_rays is the
 *    number of rays that are not degenerate; tests, hits, shadow rays and
 *    reflection rays as the reference counts them. A _device call with
 *    out == NULL only enqueues work on hip_stream; with out it waits.
 *  - flags: RT_QUERY_SORT traces the rays in rt_trace_rays' coherence order;
 *    outputs and Stats are the same byte for byte. RT_QUERY_ANY_HIT and
 *    unknown bits are RT_E_INVALID.
 * Locking and ordering are the ray queries': the call takes the scene's
 * lock, runs after a render or query still in flight on the scene, sees the
 * scene as the last rt_scene_set_lights / _set_objects / _set_mesh_vertices
 * left it, and leaves everything rt_scene_last_* reports the last render
 * call's. n == 0 is RT_OK and launches nothing; n < 0 and null required
 * pointers are RT_E_INVALID; n >= 2^31 is RT_E_UNSUPPORTED. */

/* Device form: d_orig / d_dir (n*3 doubles), d_rgb (n/group*3 doubles or
 * NULL) and d_rgb32 (n/group*3 floats or NULL) are device memory. */
int rt_shade_rays_device(rt_scene *scene, const rt_options *opts, int64_t n,
                         const double *d_orig, const double *d_dir, int32_t group,
                         uint32_t flags, double *d_rgb, float *d_rgb32,
                         void *hip_stream, rt_stats *out);
/* Host form: the same arrays in caller memory; returns with the answers. */
int rt_shade_rays(rt_scene *scene, const rt_options *opts, int64_t n,
                  const double *orig, const double *dir, int32_t group,
                  uint32_t flags, double *rgb, float *rgb32, rt_stats *out);

/* ---- float32 radiance queries --------------------------------------------
 * rt_shade_rays in the float32 mode's arithmetic, for callers that form many
 * rays per frame (a custom camera at 256 samples per pixel): float32 rays in
 * (24 bytes per ray), float32 colours out, the BVH path of the RT_FP32 render.
 *
 * Ray i is (orig[3i..], dir[3i..]), float32; dir is taken as given, NOT
 * normalised. Its colour is what the RT_FP32 render computes for a camera
 * sample with that ray: shade(ray, trace(ray)) in the arithmetic of the
 * float32 render kernel (shadow rays to distant lights keep their light-grid
 * searches, which depend on the lights and the geometry only). The scene's
 * camera is not read. Accuracy is the float32 mode's, stated
 * for bias >= 1e-4: with a bias near 1e-8 a float32 shadow ray starts inside
 * the rounding error of its own hit point and surfaces shadow themselves, as
 * INTEGRATION.md warns for RT_FP32 renders.
 *  - opts: bias, max_ray_depth, precision and flags are read. precision must
 *    be RT_FP32 (RT_FP64 is RT_E_INVALID: rt_shade_rays is the float64
 *    query). Of opts->flags only RT_FLAG_NO_BINNING is honoured — shadow rays
 *    then search the BVH instead of the light-grid cells, with the same bytes
 *    out — and every other bit is ignored. With reflective materials
 *    max_ray_depth above 7 is RT_E_UNSUPPORTED, as for a render.
 *  - group >= 1 and n % group == 0, else RT_E_INVALID; rgb holds n / group
 *    colours of three floats. group == 1: the ray's colour as computed.
 *    group > 1: starting from +0, the float32 sum of the group's colours in
 *    index order, times (float)(1.0 / (double)group) — the render's inv_len.
 *  - A degenerate ray — a non-finite component or an all-zero direction —
 *    has the colour (+0, +0, +0) and adds nothing to the Stats; it
 *    contributes +0 to its group's sum, and the group still divides by
 *    `group`. A finite ray of any magnitude never faults; where float32
 *    arithmetic overflows, its colour is unspecified and may be non-finite.
 *  - out (may be NULL) receives all five fields: num_primary_rays is the
 *    number of rays that are not degenerate, the other four are what the
 *    float32 kernels count. A _device call with out == NULL only enqueues
 *    work on hip_stream; with out it waits.
 *  - flags: RT_QUERY_SORT shades the rays in rt_trace_rays' coherence order
 *    (the keys are formed from the float values). RT_QUERY_ANY_HIT and unknown
 *    bits are RT_E_INVALID.
 *  - The colour and the Stats contribution of ray i depend on ray i, the
 *    scene and opts only: not on n, the ray's index, its neighbours in the
 *    batch, RT_QUERY_SORT, RT_FLAG_NO_BINNING, or the host versus the device
 *    form. The same holds byte for byte for group outputs.
 * Locking, ordering and edge cases are rt_shade_rays's: n == 0 is RT_OK with
 * zero Stats (group is still checked); n < 0 and null required pointers are
 * RT_E_INVALID; n >= 2^31 is RT_E_UNSUPPORTED; everything rt_scene_last_*
 * reports stays the last render call's. */

/* Device form: d_orig / d_dir (n*3 floats) and d_rgb (n/group*3 floats) are
 * device memory. */
int rt_shade_rays_f32_device(rt_scene *scene, const rt_options *opts, int64_t n,
                             const float *d_orig, const float *d_dir, int32_t group,
                             uint32_t flags, float *d_rgb, void *hip_stream, rt_stats *out);
/* Host form: the same arrays in caller memory; returns with the answers. */
int rt_shade_rays_f32(rt_scene *scene, const rt_options *opts, int64_t n,
                      const float *orig, const float *dir, int32_t group,
                      uint32_t flags, float *rgb, rt_stats *out);

/* ---- float32 ray queries -------------------------------------------------
 * rt_trace_rays and rt_pick_pixels in the float32 mode's arithmetic: float32
 * rays in (24 bytes per ray), 16-byte hits out, answered by the trace of the
 * RT_FP32 render kernel. For line-of-sight, ambient-occlusion and placement
 * batches whose answers feed float32 consumers, and for a front end that
 * displays RT_FP32 frames: rt_pick_pixels_f32 forms its ray exactly as that
 * render forms it, so the pick names the object the picture shows there
 * (the float64 pick forms a float64 ray, and may disagree at a silhouette).
 *
 * Ray i is (orig[3i..], dir[3i..]), float32; dir is taken as given, NOT
 * normalised, so t is in units of |dir|. t_near is n floats, or NULL for +inf
 * for every ray. The answer is what the float32 render's trace computes for a
 * ray with those values: the closest t with 0 <= t < t_near, the first object
 * in scene order on equal t, the lowest face index on equal t within a mesh,
 * the mesh AABB gate included (a ray that starts inside a mesh's box misses
 * that mesh). Mesh faces are searched through the BVH: no pixel list or light
 * grid of a render call is reachable. Accuracy is the float32 mode's
 * (DESIGN.md "Float32 ray queries" quotes what was measured against
 * rt_trace_rays on the same values).
 *  - Miss: obj = -1, face = -1, t = that ray's t_near.
 *  - RT_QUERY_ANY_HIT: trace as the float32 render's shadow rays call it, with
 *    their exact early exit: only obj >= 0 versus obj == -1 is meaningful
 *    (t echoes t_near, face is -1), and for every ray obj >= 0 exactly when
 *    the closest-hit query's is. normals != NULL with this flag is
 *    RT_E_INVALID.
 *  - A degenerate ray — a non-finite component, an all-zero direction or a
 *    NaN t_near — is answered as a miss with its t_near as given and adds
 *    nothing to the Stats. A finite ray of any magnitude never faults; where
 *    float32 arithmetic overflows, its answer is unspecified.
 *  - normals (may be NULL) receives three floats per ray: the N the float32
 *    render shades the hit with — normal(hitO) of a sphere, plane or box at
 *    the float32 hit point, normals[face] of a mesh hit, through
 *    objectToWorld for general transforms; not renormalised; (0, 0, 0) on a
 *    miss.
 *  - out (may be NULL): num_intersection_tests is the number of rays that are
 *    not degenerate times the scene's object count, num_intersection_hits is
 *    what the kernel counts, num_primary_rays is the number of rays that are
 *    not degenerate for a pick and 0 for a trace; the other fields are 0. A
 *    _device call with out == NULL only enqueues work on hip_stream; with out
 *    it waits for the answers.
 *  - RT_QUERY_SORT: as for rt_shade_rays_f32, the keys formed from the float
 *    values (picks: from the float image positions); hits, normals and Stats
 *    are the same, byte for byte.
 *  - The answer and the Stats contribution of ray i depend on ray i, its
 *    t_near and the scene only (picks: also on the camera, width and
 *    height): not on n, the ray's index, its neighbours in the batch,
 *    RT_QUERY_SORT, or the host versus the device form.
 * Locking, ordering and edge cases are rt_trace_rays's: n == 0 is RT_OK with
 * zero Stats; n < 0, unknown flag bits and null required pointers are
 * RT_E_INVALID; n >= 2^31 is RT_E_UNSUPPORTED; everything rt_scene_last_*
 * reports stays the last render call's. */
typedef struct rt_hit32 {   /* 16 bytes */
  float   t;                /* tHit; on a miss: that ray's t_near          */
  int32_t obj;              /* index into rt_scene_desc.objects, -1 = nil  */
  int32_t face;             /* original face index of a mesh hit, else -1  */
  int32_t reserved;         /* written as 0                                */
} rt_hit32;

/* Device form: d_orig / d_dir (n*3 floats), d_tnear (n floats or NULL),
 * d_hits (n rt_hit32, 16-byte aligned as device allocations are: RT_E_INVALID
 * otherwise) and d_normals (n*3 floats or NULL) are device memory. */
int rt_trace_rays_f32_device(rt_scene *scene, int64_t n, const float *d_orig,
                             const float *d_dir, const float *d_tnear,
                             uint32_t flags, rt_hit32 *d_hits, float *d_normals,
                             void *hip_stream, rt_stats *out);
/* Host form: the same arrays in caller memory (any alignment); returns with
 * the answers. */
int rt_trace_rays_f32(rt_scene *scene, int64_t n, const float *orig,
                      const float *dir, const float *tnear, uint32_t flags,
                      rt_hit32 *hits, float *normals, rt_stats *out);

/* Float32 picking: ray i starts at the float32 camera origin and runs along
 * the direction the RT_FP32 render forms for a sample at the float image
 * position (xy[2i], xy[2i+1]) of a width x height frame, from the same folded
 * float32 camera constants with the scene's current camera
 * (rt_scene_set_camera applies), traced with t_near = +inf. Integer (x, y) is
 * the akNone sample of that pixel, x + (i + 0.5) / m an akGrid sample;
 * fractional coordinates and coordinates outside the image are legal; a
 * non-finite coordinate makes the ray degenerate. Only width, height and
 * precision of opts are read; precision must be RT_FP32 (RT_FP64 is
 * RT_E_INVALID: rt_pick_pixels is the float64 pick). flags, hits, normals and
 * out as above; out->num_primary_rays is the number of rays that are not
 * degenerate. */
int rt_pick_pixels_f32_device(rt_scene *scene, const rt_options *opts, int64_t n,
                              const float *d_xy, uint32_t flags, rt_hit32 *d_hits,
                              float *d_normals, void *hip_stream, rt_stats *out);
int rt_pick_pixels_f32(rt_scene *scene, const rt_options *opts, int64_t n,
                       const float *xy, uint32_t flags, rt_hit32 *hits,
                       float *normals, rt_stats *out);

/* ---- feature buffers ------------------------------------------------------
 * The per-pixel feature buffers (AOVs) of an RT_FP32 frame: coverage, depth,
 * object / face id, normal and albedo, taken over the frame's own samples —
 * alpha for compositing, albedo and normal to guide a denoiser, depth for a
 * post-pass, the ids for a selection outline. One call traces the frame's
 * camera rays and shades nothing.
 *
 * Pixel (x, y) of rows [y0, y1), sample s, is the RT_FP32 render's for the
 * same width, height, aa_kind, grid_size and seed (every sampler; akGrid
 * sample s = sj*m + si sits at (x + (si+.5)/m, y + (sj+.5)/m) in float32).
 * Its ray starts at the float32 camera origin and runs along the render's
 * normalised direction, so depth is the distance from the camera. Its hit is
 * what rt_pick_pixels_f32 returns at that image position, bit for bit: t,
 * obj, face and normal. inv_len is the render's (float)(1.0 / (double)spp),
 * exactly 1 for RT_AA_NONE.
 *  - opts: width, height, aa_kind, grid_size, seed, precision and flags are
 *    read; bias and max_ray_depth are not. precision must be RT_FP32 (RT_FP64
 *    is RT_E_UNSUPPORTED); the sampler limits are a render's (grid_size
 *    outside [1, 256] is RT_E_INVALID, a (multi-)jittered grid_size above 32
 *    RT_E_UNSUPPORTED). Of flags only RT_FLAG_NO_BINNING is honoured: the
 *    camera rays then search the BVH instead of this call's per-pixel face
 *    lists and object masks. Every channel is byte-identical either way.
 *  - Rows outside [y0, y1) and NULL channels are never written. A pixel none
 *    of whose samples hits gets alpha 0, depth +inf, ids -1 and sums +0.
 *  - out (may be NULL): num_primary_rays is the number of samples traced,
 *    num_intersection_tests that times the object count,
 *    num_intersection_hits what the kernel counts (rt_pick_pixels_f32's over
 *    the same positions); shadow and reflection counts are 0. A _device call
 *    with out == NULL only enqueues work on hip_stream.
 *  - A render-class call: it takes the scene's lock, is ordered after the
 *    scene's calls in flight, and afterwards rt_scene_last_stats returns its
 *    Stats while the other rt_scene_last_* readers report nothing classified,
 *    as after an RT_FP64 render. It measures and consumes no launch order,
 *    and the next colour render gives the bytes, Stats and diagnostics it
 *    would have given without this call.
 *  - RT_E_INVALID: a null scene, opts or buffer struct; every channel NULL
 *    with y1 > y0; rows outside [0, height]. y0 == y1 is RT_OK and launches
 *    nothing. No argument error touches the device. */

/* Every pointer is width*height elements (x3 where noted), row-major as the
 * framebuffer, or NULL = not wanted. */
typedef struct rt_aov_buffers {
  float   *alpha;   /* hits * inv_len: hits = samples whose camera ray hits an object */
  float   *depth;   /* smallest tHit over the pixel's samples; +inf when none hits */
  int32_t *object;  /* rt_hit32.obj of the sample with the smallest (tHit, sample index); -1 */
  int32_t *face;    /* rt_hit32.face of that sample; -1 */
  float   *normal;  /* x3: float32 sum, from +0, over the hitting samples of the N the
                       float32 render shades the hit with (what rt_pick_pixels_f32 returns:
                       not renormalised), times inv_len */
  float   *albedo;  /* x3: the same sum of (float)rt_object_desc.albedo[c] of the hit object,
                       times inv_len */
} rt_aov_buffers;

/* Device form: the channels are device memory. */
int rt_render_aovs_device(rt_scene *scene, const rt_options *opts, const rt_aov_buffers *d_out,
                          int32_t y0, int32_t y1, void *hip_stream, rt_stats *out);
/* Host form: the channels are caller memory, staged through device buffers;
 * returns with the answers. */
int rt_render_aovs(rt_scene *scene, const rt_options *opts, const rt_aov_buffers *out_bufs,
                   int32_t y0, int32_t y1, rt_stats *out);

/* Float64 feature buffers: the same channels of an RT_FP64 frame, in float64
 * and with no tolerance anywhere — every channel of every pixel has exactly
 * one correct bit pattern.
 *
 * Pixel (x, y) of rows [y0, y1), sample s, is the RT_FP64 render's for the
 * same width, height, aa_kind, grid_size and seed: akNone at (x, y); akGrid
 * sample s = sj*m + si at x + (si * (1.0/m) + (1.0/m) * 0.5), likewise y, each
 * operation rounded to float64; the stochastic kinds at x + sx[s], y + sy[s]
 * of the pixel's sample table. Its ray is castPrimaryRay's as the RT_FP64
 * render forms it, its hit what rt_pick_pixels returns at that position, bit
 * for bit: t, obj, face and normal. inv_len is 1.0 / (double)spp.
 *  - normal and albedo start from +0.0, add the value of every hitting sample
 *    in sample-index order s = 0 .. spp-1 (calcPixel's order, renderer.nim:
 *    147-159), and are multiplied once by inv_len. The order is fixed, so the
 *    bytes do not depend on the flags, on how samples lie on the device's
 *    lanes or on the size of this call's per-pixel face lists.
 *  - opts: width, height, aa_kind, grid_size, seed, precision and flags are
 *    read; bias and max_ray_depth are not. precision must be RT_FP64 (RT_FP32
 *    is RT_E_INVALID: rt_render_aovs is that call); the sampler limits are an
 *    RT_FP64 render's. Of flags RT_FLAG_NO_BINNING (the camera rays search
 *    the BVH: no per-pixel lists or skip records) and RT_FLAG_F64_PER_LANE
 *    (one lane per pixel also where akGrid with >= 64 samples would take one
 *    pixel per wave) are honoured; every channel and the Stats are
 *    byte-identical with either set. Other bits are ignored.
 *  - Rows outside [y0, y1) and NULL channels are never written. A pixel none
 *    of whose samples hits gets alpha 0, depth +inf, ids -1 and sums +0.
 *  - out (may be NULL): as rt_render_aovs, num_intersection_hits being
 *    rt_pick_pixels' over the same positions. A _device call with out == NULL
 *    only enqueues work on hip_stream.
 *  - The call class and the RT_E_INVALID cases are rt_render_aovs': a
 *    render-class call that leaves the next colour render of either precision
 *    its bytes, Stats and diagnostics. */
typedef struct rt_aov_buffers64 {
  double  *alpha;   /* (double)hits * inv_len */
  double  *depth;   /* smallest tHit over the pixel's samples; +inf when none hits */
  int32_t *object;  /* rt_hit.obj of the sample with the smallest (tHit, sample index); -1 */
  int32_t *face;    /* rt_hit.face of that sample; -1 */
  double  *normal;  /* x3: the ordered sum of the hitNormal rt_pick_pixels returns (not
                       renormalised), times inv_len */
  double  *albedo;  /* x3: the ordered sum of rt_object_desc.albedo[c] of the hit object as
                       given, times inv_len */
} rt_aov_buffers64;

int rt_render_aovs_f64_device(rt_scene *scene, const rt_options *opts, const rt_aov_buffers64 *d_out,
                              int32_t y0, int32_t y1, void *hip_stream, rt_stats *out);
int rt_render_aovs_f64(rt_scene *scene, const rt_options *opts, const rt_aov_buffers64 *out_bufs,
                       int32_t y0, int32_t y1, rt_stats *out);

/* ---- helpers ----------------------------------------------------------- */

/* glm-style inverse of a column-major 4x4 (what geom.nim's
 * objectToWorld.inverse computes); RT_E_INVALID if singular. */
int rt_mat4_inverse(const double m[16], double out[16]);

/* .geom triangle soup (format of test/test.nim:14-26 and the writer
 * src/loaders/objconv.nim:139-153): int32 N, then N*3 vertices of 3 float32.
 * Query form: pass vertices == NULL to get *num_triangles only; then pass a
 * buffer of num_triangles*9 doubles. */
int rt_load_geom(const char *path, int64_t *num_triangles, double *vertices);

/* OBJ reader of src/loaders/obj.nim:87-126: "v x y z" and "f a b c" lines
 * (1-based indices; a 4th face vertex is ignored), other lines skipped;
 * tokens that do not parse entirely leave 0 (a coordinate) or index 0 (a
 * face vertex), as the reference's try/except defaults do — so "f 1//2 ..."
 * gives index 0 unless RT_OBJ_SLASH_INDICES takes the integer before the
 * first '/'. Face normals are not read (the reference computes them:
 * calcNormals, done by rt_scene_create when rt_mesh_desc.normals is NULL).
 * Query form: vertices == faces == NULL sets the two counts; then pass
 * buffers of num_vertices*3 doubles and num_faces*3 int32 (0-based). */
#define RT_OBJ_SLASH_INDICES 0x1u
int rt_load_obj(const char *path, uint32_t flags, int64_t *num_vertices,
                double *vertices, int64_t *num_faces, int32_t *faces);

/* objconv's writeGeom (src/loaders/objconv.nim:139-153): int32 face count,
 * then each face's three vertices as float32 x, y, z. */
int rt_write_geom(const char *path, const double *vertices,
                  int64_t num_vertices, const int32_t *faces,
                  int64_t num_faces);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_H */
