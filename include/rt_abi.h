/*
 * rt_abi.h — C ABI of the MI355X wavefront path tracer (drop-in for the
 * reference's tile renderer hot path).
 *
 * The reference (TheSandvichMaker/BUAS-Pathtracer) renders a frame as
 *   render_all_tiles (RT/raytracer.cpp:692)
 *     -> worker threads -> try_render_next_tile (:551)
 *       -> render_tile (:366) -> per pixel, per sample:
 *            scene->settings.integrator->f(&state)   (:467, advanced_integrator
 *                                                     RT/integrators.cpp:581-821)
 *            splat_filter(...)                       (:187-259)
 * into an AccumulationBuffer{w,h,frame_count,V4* pixels} (RT/Raytracer.h:44-48).
 *
 * Per-sample function pointers are far too fine-grained for a GPU, so this
 * ABI replaces the path at frame / tile-set granularity:
 * rt_render() consumes the same Scene / Material / Camera / SceneSettings /
 * FilterCache data (flattened to plain arrays: pointers become indices) and
 * fills the same float4 accumulation buffer.
 *
 * Everything here is plain C: POD structs, pointers and sizes, no C++ or
 * torch types.  Every function returns an int status (RT_OK == 0); on error
 * rt_last_error() returns a thread-local message.
 *
 * RT/ = /root/reference/Raytracer/,  MathLib/ = /root/reference/MathLib/.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8

/* ---------------------------------------------------------------- status */
enum rt_status {
    RT_OK                 = 0,
    RT_ERROR_INVALID      = 1,  /* bad argument / unsupported setting      */
    RT_ERROR_DEVICE       = 2,  /* HIP runtime failure                     */
    RT_ERROR_OUT_OF_MEMORY= 3,
    RT_ERROR_CANCELLED    = 4,  /* rt_cancel() hit during rt_render()      */
    RT_ERROR_NO_DEVICE    = 5,  /* no MI355X visible: the product path never
                                   falls back to a CPU implementation      */
};

/* ------------------------------------------------------------ math types */
typedef struct rt_v3 { float x, y, z; } rt_v3;                 /* MathLib/math_types.h:12-17 */
typedef struct rt_m4x4 { float e[4][4]; } rt_m4x4;             /* MathLib/math_types.h:43-45 */
typedef struct rt_m4x4inv { rt_m4x4 forward, inverse; } rt_m4x4inv; /* :47-50 */

/* ----------------------------------------------------------- scene model */
enum rt_material_flag {                                        /* RT/scene.h:9-13 */
    RT_MATERIAL_MIRROR   = 0x1,
    RT_MATERIAL_CHECKERS = 0x2,
    RT_MATERIAL_EMISSIVE = 0x4,
};

typedef struct rt_material {                                   /* RT/scene.h:15-29 (68 B) */
    uint32_t flags;
    rt_v3    albedo;
    rt_v3    checker_color;
    rt_v3    emission_color;
    float    ior;
    float    metallic;
    float    roughness;
    int32_t  is_participating_medium;
    rt_v3    absorb;                                           /* Medium::absorb */
} rt_material;

enum rt_primitive_type {                                       /* RT/primitives.h:3-10 */
    RT_PRIMITIVE_NONE   = 0,
    RT_PRIMITIVE_PLANE  = 1,
    RT_PRIMITIVE_SPHERE = 2,
    RT_PRIMITIVE_BOX    = 3,
    RT_PRIMITIVE_MESH   = 4,
};

typedef struct rt_primitive {                                  /* RT/primitives.h:92-106 */
    uint32_t transform_index;  /* Primitive::transform -> index into transforms[] */
    uint32_t material_id;      /* MaterialID */
    uint32_t type;             /* rt_primitive_type */
    uint32_t mesh_index;       /* RT_PRIMITIVE_MESH: index into meshes[] */
    float    p[4];             /* plane: n.xyz, d | sphere: r | box: r.xyz */
} rt_primitive;

typedef struct rt_bvh_node {                                   /* RT/bvh.h:31-37 (32 B) */
    rt_v3    bv_p;             /* centre      */
    rt_v3    bv_r;             /* half extent */
    uint32_t left_first;       /* interior: left child (right = +1); leaf: first index */
    uint16_t count;            /* > 0 => leaf */
    uint16_t split_axis;
} rt_bvh_node;

typedef struct rt_mesh {               /* RT/primitives.h:58-67 + MeshBVH RT/bvh.h:52-58 */
    uint32_t            triangle_count;
    uint32_t            has_normals;
    const rt_v3*        triangles;  /* MeshBVH::triangles: BVH order, a,b,c per triangle */
    const uint32_t*     indices;    /* MeshBVH::indices: BVH slot -> original triangle  */
    const rt_v3*        normals;    /* get_normals(mesh): ORIGINAL order, 3 per triangle */
    uint32_t            node_count;
    const rt_bvh_node*  nodes;      /* BVHStorage_Scalar layout (node 1 is padding)      */
} rt_mesh;

typedef struct rt_scene_desc {                                 /* RT/scene.h:92-120 */
    uint32_t            material_count;   const rt_material*  materials;  /* [0] null material  */
    uint32_t            primitive_count;  const rt_primitive* primitives; /* [0] null primitive */
    uint32_t            plane_count;      const rt_primitive* planes;     /* Scene::planes      */
    uint32_t            transform_count;  const rt_m4x4inv*   transforms;
    uint32_t            light_count;      const uint32_t*     lights;     /* PrimitiveIDs       */
    uint32_t            mesh_count;       const rt_mesh*      meshes;
    uint32_t            bvh_node_count;   const rt_bvh_node*  bvh_nodes;  /* Scene::bvh         */
    uint32_t            bvh_index_count;  const uint32_t*     bvh_indices;
    rt_v3               top_sky_color;
    rt_v3               bot_sky_color;
    uint32_t            skydome_w, skydome_h;
    const rt_v3*        skydome;          /* EnvironmentMap pixels (Image_V3), NULL = sky colours */
} rt_scene_desc;

typedef struct rt_camera {                                     /* RT/scene.h:31-46 */
    rt_v3 p, x, y, z;
    float vfov;
    float aspect_ratio;
    float lens_radius;
    float focus_distance;
    float film_distance;
    float half_film_w;
    float half_film_h;
} rt_camera;

enum rt_sampling_strategy {                                    /* RT/samplers.h:110-117 */
    RT_SAMPLING_UNIFORM              = 0,
    RT_SAMPLING_OPTIMIZED_BLUE_NOISE = 1,
    RT_SAMPLING_STRATIFIED           = 2,
};

enum rt_integrator {                                           /* g_integrators RT/integrators.cpp:823-830, by table index */
    RT_INTEGRATOR_ADVANCED               = 0,   /* "Advanced Pathtracer" (:581-821): NEE, MIS, roulette, media */
    RT_INTEGRATOR_WHITTED                = 1,   /* "Whitted" (:310-426): a per-scene opt-in (see below)         */
    RT_INTEGRATOR_GROUND_TRUTH_RECURSIVE = 2,   /* "Ground Truth Recursive" (:428-483): a per-scene opt-in      */
    RT_INTEGRATOR_GROUND_TRUTH_ITERATIVE = 3,   /* "Ground Truth Iterative" (:486-541): brute-force path tracer */
    RT_INTEGRATOR_NORMALS                = 4,   /* "Normals" (:544-560): first hit, 0.5*(1 + N)                 */
    RT_INTEGRATOR_DISTANCES              = 5,   /* "Distances" (:563-579): first hit, 1 - saturate(t/15)        */
    RT_INTEGRATOR_COUNT                  = 6,
};
/* The render entries take 0, 3, 4 and 5.  Whitted and Ground Truth Recursive fold their results on the way
 * back up a recursion (Whitted also branches in a medium), which a forward wavefront cannot reproduce without
 * a per-path recursion stack: they return RT_ERROR_INVALID by name, unless the scene has opted in with
 * rt_scene_set_recursive_integrators (below), which allocates that stack.  Ground Truth Iterative, Normals and
 * Distances cast no shadow rays (rt_stats::shadow_rays == 0) and ignore rt_set_env_sampling; Normals and
 * Distances trace their one camera ray whatever max_bounce_count says, as the reference's do. */

typedef struct rt_settings {                                   /* RT/scene.h:64-82 */
    int32_t  next_event_estimation;
    int32_t  importance_sample_lights;
    int32_t  importance_sample_diffuse;
    int32_t  use_mis;
    int32_t  russian_roulette;
    int32_t  caustics;
    int32_t  sampling_strategy;     /* rt_sampling_strategy */
    int32_t  use_path_guide;        /* must be 0 (dead code in the reference) */
    float    vignette_strength;
    float    lens_distortion;
    float    f_factor;
    float    diaphragm_edges;
    float    phi_shutter_max;
    uint32_t samples_per_pixel;
    uint32_t max_bounce_count;      /* <= 63: the material stack holds 64 entries */
    int32_t  integrator;            /* rt_integrator (SceneSettings::integrator) */
} rt_settings;

typedef struct rt_filter_cache {                               /* FilterCache RT/Raytracer.h:34-40 */
    uint32_t kernel_size;           /* filter radius in pixels; 0 => box (plain accumulate) */
    uint32_t cache_size;            /* 256 when a kernel is loaded, 0 for the box filter    */
    float    cache[512];            /* load_reconstruction_kernel RT/raytracer.cpp:164-185 */
} rt_filter_cache;

typedef struct rt_accumulation_buffer {                        /* RT/Raytracer.h:44-48 */
    uint32_t w, h;
    uint32_t frame_count;
    float*   pixels;                /* w*h float4 (xyz = weighted radiance, w = weight) */
} rt_accumulation_buffer;

typedef struct rt_post_settings {   /* PostProcessSettings RT/scene.h:84-90 */
    float   exposure;               /* stops: colour *= 2^exposure when != 0 */
    int32_t tonemapping;            /* 1 - exp(-x) */
    int32_t srgb_transform;         /* x^(1/2.23333) */
    float   midpoint;               /* sigmoidal_contrast (RT/raytracer.cpp:69-84) */
    float   contrast;
} rt_post_settings;

typedef struct rt_tile_set {        /* WorkQueue tiling RT/Raytracer.h:70-91 + sharding */
    uint32_t tile_w, tile_h;        /* 64x64 in the reference (RT/raytracer.cpp:1657) */
    uint32_t shard_index;           /* this GPU renders tiles t with t % shard_count == shard_index */
    uint32_t shard_count;
} rt_tile_set;

enum rt_rng_mode {
    /* One xorshift RandomSeries per sample, seeded from
     * (total_frame_index, frame_count, tile_index, pixel, sample): the draw
     * order inside a sample is exactly the reference's.  The GPU path. */
    RT_RNG_PER_SAMPLE  = 0,
    /* One RandomSeries per 64x64 tile consumed serially in pixel/sample order,
     * exactly RT/raytracer.cpp:588-593 (CPU oracle only). */
    RT_RNG_TILE_STREAM = 1,
};

enum rt_kernel_id {                 /* wavefront stages, for rt_stats::kernel_ms */
    RT_KERNEL_GENERATE = 0,         /* camera rays (render_tile ray setup)               */
    RT_KERNEL_EXTEND   = 1,         /* closest hit (intersect_scene)                     */
    RT_KERNEL_SHADE    = 2,         /* one bounce of advanced_integrator                 */
    RT_KERNEL_CONNECT  = 3,         /* shadow rays (intersect_shadow_ray)                */
    RT_KERNEL_SPLAT    = 4,         /* finished samples -> records (or atomic splat)     */
    RT_KERNEL_RESOLVE  = 5,         /* splat_filter as a gather in reference order       */
    RT_KERNEL_COUNT    = 6,
};

/* The reference's TraversalStats (RT/intersection.h:33-40): render_all_tiles hands them to its
 * caller and zeroes them every frame (RT/raytracer.cpp:727-731); intersect_mesh counts them
 * (RT/intersection.cpp:254, :378-380).  Here they are counted on the device, per frame, in this
 * library's own walk, whose order and layout differ from the reference's in two documented ways
 * (DESIGN.md section 3):
 *   - the top level is walked in one fixed order with the planes, spheres and boxes tested before
 *     any mesh BVH (the hits are the reference's), so t at a top-level node does not yet include
 *     the mesh hits the reference's front-to-back walk would have found;
 *   - mesh BVHs are BVH4s (each BVH2 interior node merged with its interior children), and a child
 *     is box-tested when its parent is expanded instead of when it is popped.
 * A shadow query that a mesh occludes is counted like any other (the reference returns before its
 * traversal counts are added, RT/intersection.cpp:297-299).
 * So these values are NOT comparable to the reference's own TraversalStats for the same frame (C3:
 * mesh_bvh_traversals 3.6 G BVH4 steps against the reference's 10.4 G BVH2 pops); tests pin them
 * against the oracle's restatement of this library's walk (tests/test_gpu_fullscale.py). */
typedef struct rt_traversal_stats {
    /* intersect_mesh calls (RT/intersection.cpp:488, counted at :254): mesh instances a query's
       top-level walk reaches -- the top-level leaf holding the instance passes its pop-time test
       (:454), the instance is not the query's ignored light (:466), and no plane, sphere or box has
       occluded a shadow query before it */
    uint64_t mesh_intersection_count;
    /* mesh BVH steps: each one round of 8 x 16-byte loads per lane -- an instance's entry (its
       object-space ray, RT/intersection.cpp:472, and its root box test), a BVH4 interior node, or up
       to two triangles of a leaf.  (Reference: BVH2 nodes taken from the stack, :274.) */
    uint64_t mesh_bvh_traversals;
    /* BVH4 interior nodes expanded: taken from the stack with their far-clip test passed.
       (Reference: BVH2 interior nodes that pass their pop-time test, :358.) */
    uint64_t mesh_node_traversals;
    /* mesh BVH leaves entered: taken from the stack with their far-clip test passed -- the
       reference's definition (:279); the BVH4 has the BVH2's leaves */
    uint64_t mesh_leaf_traversals;
} rt_traversal_stats;

typedef struct rt_stats {
    uint64_t closest_hit_rays;      /* intersect_scene calls (RT/integrators.cpp:615)      */
    uint64_t shadow_rays;           /* intersect_shadow_ray calls (RT/integrators.cpp:756) */
    uint64_t samples;               /* camera samples integrated                            */
    uint64_t iterations;            /* wavefront iterations (GPU) / 0 (CPU)                 */
    double   seconds;               /* wall time of the render call                         */
    /* filled only while rt_set_profiling(1): HIP-event time per stage, summed over
       launches, measured on the stream the stage kernels run on */
    double   kernel_ms[RT_KERNEL_COUNT];
    uint64_t kernel_launches[RT_KERNEL_COUNT];
    /* rays handed to the trace kernels (closest, shadow): the rest were settled by
       the planes / top-level root test where they were made (GPU only) */
    uint64_t traced_rays[2];
    int32_t  splat_mode;            /* rt_splat_mode the frame used (rt_render / rt_render_device) */
    int32_t  shadow_launch;         /* (ABI 8) rt_shadow_launch the frame used: SEPARATE or MERGED */
    /* TraversalStats of the frame (above) per query kind: [0] closest-hit (intersect_scene),
       [1] shadow (intersect_shadow_ray); the reference's totals are the sums of the two */
    rt_traversal_stats traversal[2];
    /* trace steps per kind of the extend / connect kernels (top-level steps included; r05: the fused
       drain's steps, which the TraversalStats above include, are left out, so that the steps match the
       launches bench.py times): the fetch rounds of 128 B per lane the traversal roofline counts */
    uint64_t trace_steps[2];
    /* (ABI 7) The reference's own TraversalStats units, filled only when rt_scene_config::traversal_ref
       is set (zero otherwise): per query kind, intersect_mesh calls and the BVH2 counts of the
       reference's walk -- nodes taken from the stack (RT/intersection.cpp:274), interior nodes (:358)
       and leaves (:279) passing their pop-time test -- with its top-level order and its early return
       (a shadow query that a mesh occludes adds no traversal counts, :297-299).  These are the numbers
       the reference's UI prints (RT/raytracer.cpp:2050-2056); tests/test_gpu_fullscale.py holds them to
       the oracle's reference walk of the same frame. */
    rt_traversal_stats traversal_ref[2];
} rt_stats;

typedef struct rt_ray_query {       /* debug/parity entry: one ray for rt_debug_intersect */
    rt_v3    o, d;
    float    max_t;
    uint32_t ignored_primitive;     /* 0 for closest hit; light id for shadow rays */
} rt_ray_query;

typedef struct rt_hit_record {
    float    t;
    uint32_t primitive;             /* primitive index, or RT_HIT_PLANE_BIT|plane index; 0xFFFFFFFF = miss */
    rt_v3    hit_p;
    rt_v3    n;
} rt_hit_record;

#define RT_HIT_MISS       0xFFFFFFFFu
#define RT_HIT_PLANE_BIT  0x80000000u

/* ------------------------------------------------------------ functions */
typedef struct rt_scene rt_scene;   /* device-resident scene (opaque) */

int         rt_abi_version(void);
const char* rt_last_error(void);
int         rt_device_count(int* out_count);

/* The reference's integrator table (g_integrators, RT/integrators.cpp:823-830).  rt_integrator_name: the
 * name its UI lists for a table index, NULL when out of range.  rt_find_integrator: the index of a name,
 * 0 (the default integrator) when unknown, as find_integrator (:835-845).  rt_integrator_supported: 1 when
 * the render entries take the index, else 0.  None needs a device. */
const char* rt_integrator_name(int integrator);
int         rt_find_integrator(const char* name);
int         rt_integrator_supported(int integrator);

/* Whitted and Ground Truth Recursive as a per-scene opt-in.  rt_scene_set_recursive_integrators(scene, 1):
 * rt_render, rt_render_device, rt_render_picture and rt_trace_samples take integrators 1 and 2 for this
 * scene; it allocates a frame stack on the scene's device (64 levels of 48 bytes per lane of a persistent
 * kernel that fills the GPU: 384 MiB on an MI355X), which (scene, 0) or rt_scene_free releases.  Off
 * (the default) they return RT_ERROR_INVALID as before.  Their frames run as one partition, a camera sample
 * per lane walked depth-first; Whitted makes two calls at every hit on a participating medium, so its cost
 * doubles per medium bounce: keep max_bounce_count small where a medium is visible.
 * rt_scene_integrator_supported: rt_integrator_supported plus 1 and 2 when the scene has the opt-in on; with
 * a NULL scene it equals rt_integrator_supported.
 * rt_scene_set_ambient_light: Scene::ambient_light (RT/scene.h:102), which only Whitted reads
 * (RT/integrators.cpp:371); rt_scene_desc has no such field.  Default (0, 0, 0). */
int rt_scene_set_recursive_integrators(rt_scene* scene, int enable);
int rt_scene_integrator_supported(const rt_scene* scene, int integrator);
int rt_scene_set_ambient_light(rt_scene* scene, const rt_v3* ambient_light);

/* Upload a flattened scene to `device` (create_scene_bvh must have run on
 * the host: RT/scene.cpp:173-242).  The device copy is owned by *out. */
int rt_scene_upload(const rt_scene_desc* desc, int device, rt_scene** out);
int rt_scene_free(rt_scene* scene);

/* Render one progressive frame: the equivalent of render_all_tiles releasing
 * its workers over every tile of `tiles` (RT/raytracer.cpp:692-757), with
 * accum->frame_count as the canonical sample base (RT/raytracer.cpp:427-428).
 * accum->pixels is HOST memory; samples are ADDED to it (the caller resets it
 * exactly as reset() does, RT/raytracer.cpp:511-515). */
int rt_render(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
              const rt_filter_cache* filter, const rt_tile_set* tiles,
              uint32_t total_frame_index, rt_accumulation_buffer* accum, rt_stats* stats);

/* Same, but d_pixels is a DEVICE pointer (w*h float4 on the scene's device)
 * and `hip_stream` (hipStream_t, may be NULL) is the stream the work is
 * ordered on.  Returns after the frame has completed on the device. */
int rt_render_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                     const rt_filter_cache* filter, const rt_tile_set* tiles,
                     uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                     float* d_pixels, void* hip_stream, rt_stats* stats);

/* The frame of the reference's "Take picture" (RT/raytracer.cpp:2031-2048, :2089-2176):
 * renders total_frame_index's frame of settings->samples_per_pixel samples per pixel
 * into a fresh device buffer (frame_count 0), then runs the output pass on the device
 * (rt_postprocess_device) with the dither texture of total_frame_index + 1 -- the frame
 * completing advances the index before the output pass reads it (:720-724, :2108) -- and
 * copies the BGRA8 picture (w*h u32, host) out.  write_bitmap is the caller's. */
int rt_render_picture(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                      const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                      uint32_t w, uint32_t h, const rt_post_settings* post, uint32_t* out_bgra, rt_stats* stats);

/* Parity entry: integrate an explicit list of samples (pixel x,y + sample
 * offset s, canonical index = frame_count + s) with RT_RNG_PER_SAMPLE and
 * return, per sample, {r, g, b, jitter_x, jitter_y} (radiance after
 * vignetting, the value splat_filter receives).  Host pointers. */
int rt_trace_samples(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                     uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                     uint32_t frame_count, uint32_t total_frame_index,
                     uint32_t count, const uint32_t* pixel_xy, const uint32_t* sample_offset,
                     float* out_rgbjj, rt_stats* stats);

/* Parity entry: intersect_scene (closest hit, occlusion = 0) or
 * intersect_shadow_ray (occlusion = 1) for `count` rays (RT/intersection.cpp:600-610). */
int rt_debug_intersect(rt_scene* scene, uint32_t count, const rt_ray_query* rays,
                       int occlusion, rt_hit_record* out);

/* Verification entries for the device layouts built at rt_scene_upload (host only,
 * no device needed).  rt_debug_mesh_bvh4: the BVH4 a mesh BVH2 (the caller's
 * BVHNode array, RT/bvh.h:31-37) is traversed as, 8 x float4 per node (SoA
 * children: p.x[4] p.y[4] p.z[4] r.x[4] r.y[4] r.z[4], packed records[4], split
 * axes); interior records are node indices, leaf records bit 30 | count << 25 |
 * first, 0xFFFFFFFF no child.  rt_debug_top_sequences: the top level as the ray
 * prologue walks it, per direction octant (bit k = d[k] < 0) node_count entries of
 * 2 x float4 {bv_p, bv_r.x}, {bv_r.yz, leaf info (0x80000000 | count << 24 | first,
 * 0 interior), skip (the entry after the subtree)}.  Both return RT_ERROR_INVALID
 * when the tree does not fit the layout, and write the counts they need. */
int rt_debug_mesh_bvh4(const rt_bvh_node* nodes, uint32_t node_count, float* out, uint32_t out_cap_nodes,
                       uint32_t* out_nodes, uint32_t* out_root_record);
int rt_debug_top_sequences(const rt_bvh_node* nodes, uint32_t node_count, uint32_t index_count,
                           float* out, uint32_t out_cap_entries, uint32_t* out_len);

/* The claim -> slot mapping of the path generation (host only, no device needed).  A
 * pool of `nwaves` waves of 64 slots (a multiple of 4: blocks of 256) where wave w's
 * last free_w[w] (<= 64) slots are free: the new paths of an iteration claim the free
 * slots in slot order.  Writes the slots of the claims [first_claim, first_claim +
 * count), found the way the generate kernel finds them, in waves of 64 claims from
 * first_claim on.  RT_ERROR_INVALID when the range passes the free slots. */
int rt_debug_claim_slots(const uint32_t* free_w, uint32_t nwaves, uint32_t first_claim, uint32_t count,
                         uint32_t* out_slots);
/* The mirror of it, the rank -> slot mapping of the dense ramp-down shade (host only): the same
 * pool, whose alive paths are wave w's first 64 - free_w[w] slots, ranked in slot order.  Writes
 * the slots of the ranks [first_rank, first_rank + count), found the way the shade kernel finds
 * them, in waves of 64 ranks from first_rank on.  RT_ERROR_INVALID when the range passes the
 * alive paths. */
int rt_debug_rank_slots(const uint32_t* free_w, uint32_t nwaves, uint32_t first_rank, uint32_t count,
                        uint32_t* out_slots);
/* The ramp-down of the scene's last frame, summed over its partitions: the shade iterations that
 * ran after the last sample was claimed and before the fused drain (or the frame's end), and the
 * paths they shaded.  iterations x the path pool - paths is the slots those launches found empty. */
int rt_scene_ramp_stats(const rt_scene* scene, uint64_t* out_iterations, uint64_t* out_paths);

/* Exhaustive check of the kernels' fast reciprocal (3 instructions instead of the
 * division expansion) against the correctly rounded IEEE 1.0f / x on `device`: every
 * one of the 2^32 bit patterns (NaNs compare equal as NaNs).  Writes the number of
 * mismatching inputs and the smallest mismatching bit pattern (0xFFFFFFFF: none). */
int rt_debug_verify_rcp(int device, uint64_t* out_mismatches, uint32_t* out_first_bits);

/* The same for the kernels' division by the constant PI (3 instructions: an estimate
 * and one residual correction) against the IEEE x / 3.14159265359f: every one of the
 * 2^32 bit patterns. */
int rt_debug_verify_div_pi(int device, uint64_t* out_mismatches, uint32_t* out_first_bits);

/* The kernels' division of three numerators by one denominator (the division
 * expansion with the denominator's part done once) against three IEEE divisions, bitwise
 * (NaNs compare equal as NaNs), for `count` sets of 4 floats: numerators x, y, z and the
 * denominator.  Writes the number of mismatching sets and the index of the first
 * (0xFFFFFFFF: none). */
int rt_debug_verify_div3(int device, uint32_t count, const float* sets, uint64_t* out_mismatches,
                         uint32_t* out_first_index);

/* The output pass of RT/raytracer.cpp:2103-2171 on the device: per pixel resolve
 * (xyz / w), exposure, 1-exp(-x) tonemap, sRGB power, sigmoidal contrast, x255,
 * TPDF dither from the reference's LDR_RGB1 blue-noise texture number
 * total_frame_index % 8 (RT/assets.cpp:63-113), clamp, BGRA8 pack; NaN pixels
 * become (0,255,255), negative weights magenta.  d_pixels (w*h float4) and d_bgra
 * (w*h u32) are DEVICE pointers on `device`; `hip_stream` may be NULL.
 * remap_tpdf's rsqrtss (an approximation whose bits differ between CPU models)
 * is computed as 1/sqrt, correctly rounded. */
int rt_postprocess_device(int device, const float* d_pixels, uint32_t w, uint32_t h,
                          const rt_post_settings* post, uint32_t total_frame_index,
                          uint32_t* d_bgra, void* hip_stream);

/* Same, from and to host memory (accum->pixels in, out_bgra w*h u32 out). */
int rt_postprocess(int device, const rt_accumulation_buffer* accum, const rt_post_settings* post,
                   uint32_t total_frame_index, uint32_t* out_bgra);

/* The denoise stage: an edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010)
 * between an accumulation buffer and the output pass.  Beyond the reference, which has no denoiser: an
 * opt-in that no other entry calls.  DESIGN.md ("The denoise stage") defines it operation by operation;
 * the device matches the plain-C restatement tests/ref_denoise/ref_denoise.c bit for bit.  In short:
 *   - beauty and the (up to two, either may be NULL) guide buffers are w*h float4 accumulation buffers
 *     (sum w*rgb, sum w), resolved per pixel as the output pass resolves: xyz / w when w > 0.001f;
 *   - a pixel is valid when its beauty weight is > 0.001f, its resolved colour is finite, and every guide
 *     that is present has a weight > 0.001f and a finite resolved value there.  Invalid pixels come out
 *     as they went in (all four floats: the output pass still shows NaN as cyan and a negative weight as
 *     magenta) and contribute to no neighbour;
 *   - the resolved colour is clamped to [0, firefly_clamp] per channel (no upper clamp when 0);
 *   - iteration i of `iterations` runs the 5x5 B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16}^2 with holes
 *     at step 2^i, each tap weighted by expf(-e), e = (l(p) - l(q))^2 / (sigma_color 2^-i)^2
 *     + sum_k |g_k(p) - g_k(q)|^2 / sigma_guide[k]^2, where l = 1 - expf(-luminance) of the current colour
 *     (Rec. 709 weights) and g_k the resolved guide values; taps outside the image or invalid are skipped
 *     and the weights renormalised;
 *   - a valid pixel comes out as {r, g, b, 1.0f}, so rt_postprocess_device takes the buffer as it is.
 * rt_denoise_default_params: 3 iterations, sigma_color 1.0, sigma_guide {0.1, 0.05} (guide 0 = a Normals
 * frame, guide 1 = a Distances frame, integrators 4 and 5), firefly_clamp 10. */
typedef struct rt_denoise_params {
    int32_t iterations;        /* 1..8 */
    float   sigma_color;       /* tonemapped-luminance term, halved per iteration; 0 = off */
    float   sigma_guide[2];    /* per guide buffer; 0 = term off */
    float   firefly_clamp;     /* per-channel clamp of the resolved radiance before filtering; 0 = none */
    int32_t reserved[3];
} rt_denoise_params;
int    rt_denoise_default_params(rt_denoise_params* out);                 /* no device needed */
size_t rt_denoise_workspace_bytes(uint32_t w, uint32_t h);                /* 64 bytes per pixel; no device needed */
/* Device pointers on `device` (w*h float4 each); d_out may equal d_beauty.  d_workspace holds
 * rt_denoise_workspace_bytes(w, h) bytes; with NULL the call allocates and frees its own.  `hip_stream` may
 * be NULL; returns after the filter has completed.  RT_ERROR_INVALID, naming the field, for a NULL beauty,
 * parameter or output pointer, w or h of 0, iterations outside 1..8, a negative or non-finite sigma or
 * clamp, and a non-zero sigma_guide[k] whose guide is NULL: all checked before the device is touched. */
int rt_denoise_device(int device, const float* d_beauty, const float* d_guide0, const float* d_guide1,
                      uint32_t w, uint32_t h, const rt_denoise_params* p, void* d_workspace,
                      float* d_out, void* hip_stream);
/* Same, from and to host memory (beauty->pixels, guide0, guide1 in; out_pixels w*h float4 out).
 * RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_denoise(int device, const rt_accumulation_buffer* beauty, const float* guide0, const float* guide1,
               const rt_denoise_params* p, float* out_pixels);
/* rt_render_picture with the denoise stage, written on the public entries: fresh device buffers; the beauty
 * frame as rt_render_picture renders it (the caller's settings, frame_count 0); a Normals and a Distances
 * frame of guide_spp samples per pixel (0: the beauty frame's count) with the same camera, filter, tiles
 * and total_frame_index; rt_denoise_device with guide 0 = normals and guide 1 = distances;
 * rt_postprocess_device with the dither texture of total_frame_index + 1.  `stats` is the beauty frame's. */
int rt_render_picture_denoised(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                               const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                               uint32_t w, uint32_t h, const rt_post_settings* post, const rt_denoise_params* p,
                               uint32_t guide_spp, uint32_t* out_bgra, rt_stats* stats);

/* Feature frames: what a pixel shows at the end of its specular prefix.  Beyond the reference; an opt-in
 * beside the integrators (rt_settings::integrator is ignored, the integrator table keeps its six rows).
 * The sample and its camera ray are the beauty frame's (the same key, the same sampler draws, the same
 * vignette).  The walk is the Advanced integrator cut off at its first non-specular vertex: at each hit,
 * inside / outside and the material stack as that integrator; T += t; the walk ends when the material
 * entered is emissive, when the Fresnel test takes the diffuse branch of a material that is no
 * participating medium, or at hit number max(max_bounce_count, 1); otherwise it reflects or refracts as
 * the integrator does (its Sample_Reflectance and random_in_unit_sphere draws, no others) and goes on.
 *   RT_FEATURE_NORMAL    0.5*(1 + N), N as the intersection returns it (integrator 4's value)
 *   RT_FEATURE_DISTANCE  1 - saturate(T/15) as a grey (integrator 5's value, of the accumulated distance)
 *   RT_FEATURE_ALBEDO    evaluate_material at the diffuse vertex (checkers included); (1, 1, 1) on an
 *                        emitter, at the bound on a specular vertex, and on a miss
 * On a miss NORMAL and DISTANCE are the sky of the last direction.  No NEE, no shadow ray, no roulette:
 * rt_stats::shadow_rays is 0 and closest_hit_rays - samples counts the specular bounces followed.  With
 * max_bounce_count <= 1 the NORMAL and DISTANCE frames are integrator 4's and 5's, bit for bit.
 * DESIGN.md ("Feature frames") defines the walk operation by operation; the device matches the plain-C
 * restatement tests/ref_features/ref_features.c bit for bit in the exact splat mode. */
enum rt_feature { RT_FEATURE_NORMAL = 0, RT_FEATURE_DISTANCE = 1, RT_FEATURE_ALBEDO = 2, RT_FEATURE_COUNT = 3 };
/* Arguments and accumulation as rt_render_device.  A `feature` outside rt_feature is RT_ERROR_INVALID,
 * named, before the device is touched. */
int rt_render_feature_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                             const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                             uint32_t w, uint32_t h, uint32_t frame_count, int feature, float* d_pixels,
                             void* hip_stream, rt_stats* stats);
/* Same, into host memory, as rt_render. */
int rt_render_feature(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                      const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                      int feature, rt_accumulation_buffer* accum, rt_stats* stats);
/* The three feature frames in one walk.  Arguments and accumulation as rt_render_feature_device; samples are
 * added to each buffer, and after the call buffer f holds what rt_render_feature_device(..., feature = f, ...)
 * would have added to it: the same records, resolved once per buffer, so in the exact splat mode (and in the
 * streaming mode under one configuration) the three equal the single-feature frames bit for bit.  The camera
 * rays, the specular bounces and the frame's ramp-down run once: `stats` describes that one walk (samples and
 * closest_hit_rays are a single feature frame's, shadow_rays is 0).  A sample leaves three 20-byte records,
 * so the record budget counts three rings: over it the exact mode streams and the rings shorten, as for any
 * frame.  All three buffers are required and must be distinct; a NULL scene, camera, settings, filter, tiles or
 * buffer, two equal buffers and a w or h of 0 are RT_ERROR_INVALID, each named, before the device is touched. */
int rt_render_features_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                              const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                              uint32_t w, uint32_t h, uint32_t frame_count, float* d_normal, float* d_distance,
                              float* d_albedo, void* hip_stream, rt_stats* stats);
/* Same, into host memory, as rt_render_feature.  The three buffers must agree in w, h and frame_count
 * (RT_ERROR_INVALID, named).  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_render_features(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                       const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                       rt_accumulation_buffer* normal, rt_accumulation_buffer* distance,
                       rt_accumulation_buffer* albedo, rt_stats* stats);

/* The denoise stage with feature frames: rt_denoise_device's filter (guide 0 = a NORMAL frame, guide 1 = a
 * DISTANCE frame) with an albedo frame, which
 *   - resolves as the guides do and, when present, takes part in the validity rule like a guide;
 *   - with `demodulate`, divides the clamped colour per channel by a = max(albedo, albedo_floor) before
 *     the first iteration (l is taken of the demodulated colour) and multiplies it back after the last;
 *   - with sigma_albedo > 0, adds |albedo(p) - albedo(q)|^2 / sigma_albedo^2 to a tap's e after the two
 *     guide terms.
 * With the albedo NULL, demodulate 0 and sigma_albedo 0 the output is rt_denoise_device's, bit for bit.
 * The workspace is 80 bytes per pixel.  Refusals as rt_denoise_device, and by name: demodulate or
 * sigma_albedo > 0 with a NULL albedo, a negative or non-finite sigma_albedo, demodulate outside 0 / 1,
 * and with demodulate an albedo_floor that is not finite and > 0. */
typedef struct rt_denoise_features_params {
    rt_denoise_params base;   /* guide 0 = NORMAL, guide 1 = DISTANCE */
    float   sigma_albedo;     /* edge-stopping term on the resolved albedo; 0 = off */
    int32_t demodulate;       /* 0 / 1 */
    float   albedo_floor;     /* > 0 and finite when demodulate */
    int32_t reserved[5];
} rt_denoise_features_params;
int    rt_denoise_features_default_params(rt_denoise_features_params* out);      /* no device needed */
size_t rt_denoise_features_workspace_bytes(uint32_t w, uint32_t h);              /* 80 bytes per pixel; no device needed */
int rt_denoise_features_device(int device, const float* d_beauty, const float* d_normal, const float* d_distance,
                               const float* d_albedo, uint32_t w, uint32_t h, const rt_denoise_features_params* p,
                               void* d_workspace, float* d_out, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_denoise_features(int device, const rt_accumulation_buffer* beauty, const float* normal, const float* distance,
                        const float* albedo, const rt_denoise_features_params* p, float* out_pixels);
/* rt_render_picture_denoised with feature frames, written on the public entries: the beauty frame; a
 * NORMAL, a DISTANCE and an ALBEDO frame of guide_spp samples per pixel (0: the beauty frame's count) with
 * the same camera, filter, tiles, total_frame_index and max_bounce_count (rendered in one walk by
 * rt_render_features_device: the three rt_render_feature_device frames, bit for bit); rt_denoise_features_device;
 * rt_postprocess_device with the dither texture of total_frame_index + 1.  `stats` is the beauty frame's. */
int rt_render_picture_features_denoised(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                        const rt_filter_cache* filter, const rt_tile_set* tiles,
                                        uint32_t total_frame_index, uint32_t w, uint32_t h,
                                        const rt_post_settings* post, const rt_denoise_features_params* p,
                                        uint32_t guide_spp, uint32_t* out_bgra, rt_stats* stats);

/* Adaptive sampling by tiles: frames over an explicit tile list, a per-tile error estimate, and a driver that
 * loops the two until every tile is under a threshold or has taken max_spp samples.  Beyond the reference,
 * which gives every pixel samples_per_pixel samples: an opt-in of new entries only (no existing struct or
 * entry changes; RT_ABI_VERSION stays).  DESIGN.md ("Adaptive sampling by tiles") defines all three; the
 * error estimate matches the plain-C restatement tests/ref_adaptive/ref_adaptive.c bit for bit.
 *
 * 1. rt_render_tiles_device: rt_render_device for the tiles of `tile_ids` (tile_count indices into the
 * reference's tile grid: tile t is column t % tcx, row t / tcx, tcx = ceil(w / tile_w)) instead of a shard's.
 * The listed tiles are rendered in descending order, the reference's queue order, and their samples splat into
 * every pixel the filter reaches, halos into unlisted tiles included.  A sample's key is (total_frame_index,
 * frame_count, tile, pixel, sample) as ever, so a tile rendered alone draws the samples the whole frame draws
 * there.  Any integrator the scene supports; sharding does not apply (no rt_tile_set; rt_set_shard_mode has no
 * meaning here).  tile_count == 0 is RT_OK with zeroed stats.  RT_ERROR_INVALID, naming the field, before the
 * device is touched: w, h, tile_w or tile_h of 0, a NULL list with tile_count > 0, an id >= tcx*tcy, a list
 * that is not strictly ascending (a duplicate included), and a NULL scene, camera, settings, filter or buffer
 * (checked in this order: the list's checks need no scene). */
int rt_render_tiles_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                           const rt_filter_cache* filter, uint32_t tile_w, uint32_t tile_h,
                           const uint32_t* tile_ids, uint32_t tile_count, uint32_t total_frame_index,
                           uint32_t w, uint32_t h, uint32_t frame_count, float* d_pixels, void* hip_stream,
                           rt_stats* stats);
/* Same, into host memory, as rt_render (w, h and frame_count are accum's). */
int rt_render_tiles(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                    const rt_filter_cache* filter, uint32_t tile_w, uint32_t tile_h,
                    const uint32_t* tile_ids, uint32_t tile_count, uint32_t total_frame_index,
                    rt_accumulation_buffer* accum, rt_stats* stats);

/* 2. rt_tile_error_device: the half-buffer error of Dammertz et al. (HPG 2010; Cycles' criterion too) per
 * tile.  A and B are two w*h float4 accumulation buffers (sum w*rgb, sum w) holding disjoint halves of the
 * samples.  Per pixel of a tile: valid when both weights are > 0.001f and all eight floats are finite;
 *   a = A.xyz / A.w,  b = B.xyz / B.w,  m = (A.xyz + B.xyz) / (A.w + B.w),
 *   e = (|a.r - b.r| + |a.g - b.g| + |a.b - b.b|) / sqrtf(max(m.r + m.g + m.b, floor)).
 * Per tile: tile_error = sum e / n_valid (+INFINITY when no pixel is valid, so a threshold never retires the
 * tile) and tile_valid = n_valid.  d_tile_ids (device, tile_count ids < tcx*tcy in any order) or NULL for
 * every tile (tile_count must then be tcx*tcy); the outputs (device) are indexed by position in the list.
 * One workgroup per tile and one fixed summation order: a pure function of the two buffers.
 * RT_ERROR_INVALID by name for a NULL buffer, parameter or output pointer, w, h, tile_w or tile_h of 0, a
 * tile_count of 0 or above tcx*tcy (or other than tcx*tcy with a NULL list), and a floor that is not finite
 * and > 0: all before the device is touched.  An id out of range on the device gives +INFINITY and 0. */
typedef struct rt_tile_error_params {
    float   floor;             /* lower bound of m.r + m.g + m.b under the root; default 1e-4f */
    int32_t reserved[3];
} rt_tile_error_params;
int rt_tile_error_default_params(rt_tile_error_params* out);               /* no device needed */
int rt_tile_error_device(int device, const float* d_half_a, const float* d_half_b, uint32_t w, uint32_t h,
                         uint32_t tile_w, uint32_t tile_h, const uint32_t* d_tile_ids, uint32_t tile_count,
                         const rt_tile_error_params* p, float* d_tile_error, uint32_t* d_tile_valid,
                         void* hip_stream);
/* Same, from and to host memory (tile_ids host or NULL; the list's ids are checked on the host).
 * RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_tile_error(int device, const float* half_a, const float* half_b, uint32_t w, uint32_t h,
                  uint32_t tile_w, uint32_t tile_h, const uint32_t* tile_ids, uint32_t tile_count,
                  const rt_tile_error_params* p, float* tile_error, uint32_t* tile_valid);

/* 3. rt_render_adaptive_device: written on the two above.  settings->samples_per_pixel is ignored; max_spp
 * rules.  The active list starts as every tile.  Round r = 0, 1, ... while tiles are active and
 * r*step_spp < max_spp: the active list is rendered into half buffer A with frame_count + r*step_spp and
 * step_spp/2 samples, and into half buffer B with frame_count + r*step_spp + step_spp/2 and step_spp/2
 * samples (rt_render_tiles_device both: together the samples a uniform frame of step_spp samples at
 * frame_count + r*step_spp draws in those tiles); once (r+1)*step_spp >= min_spp, rt_tile_error_device runs
 * over the active list, the errors are read back, and tiles with error <= threshold leave the list.  At the
 * end one kernel adds A + B into d_pixels (samples are added, as in every render entry).  out_tile_spp[t]
 * (host, tcx*tcy, may be NULL) is the samples tile t took.  The counters of `stats` are sums over the calls,
 * `seconds` the wall time of the whole call, splat_mode and shadow_launch the last frame's.  rt_cancel ends
 * the loop with RT_ERROR_CANCELLED (d_pixels is then untouched).  The workspace is two w*h float4 buffers and
 * the per-tile lists (rt_adaptive_workspace_bytes); with NULL the call allocates and frees its own.
 * RT_ERROR_INVALID by name before the device is touched: a NULL parameter, scene, camera, settings, filter or
 * buffer; step_spp 0 or odd; min_spp or max_spp of 0 or no multiple of step_spp; min_spp > max_spp; a
 * threshold that is negative or not finite; a bad error floor; w, h, tile_w or tile_h of 0.
 * rt_adaptive_default_params: min_spp 16, max_spp 256, step_spp 16, floor 1e-4f, and threshold 0.5f: the value
 * at which C3 at 480x270 takes the samples of a 64 to 128 spp uniform frame (DESIGN.md section 6 has the table).
 * It is a budget, not a quality claim: at equal samples the uniform frame measured as good or better on C3 and
 * C4, so choose the threshold per scene.  A frame costs about 2.4 ms whatever it renders, so a round (two
 * frames and an estimate) should carry some millions of samples: raise step_spp for frames under 1080p. */
typedef struct rt_adaptive_params {
    uint32_t min_spp, max_spp, step_spp;   /* step_spp even and > 0; min_spp <= max_spp; both multiples of step_spp */
    float    threshold;                    /* a tile retires when its error <= threshold; >= 0, finite */
    rt_tile_error_params error;
    int32_t  reserved[4];
} rt_adaptive_params;
int    rt_adaptive_default_params(rt_adaptive_params* out);                                     /* no device needed */
size_t rt_adaptive_workspace_bytes(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h);   /* no device needed */
int rt_render_adaptive_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                              const rt_filter_cache* filter, uint32_t tile_w, uint32_t tile_h,
                              uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                              const rt_adaptive_params* p, void* d_workspace, float* d_pixels,
                              uint32_t* out_tile_spp, void* hip_stream, rt_stats* stats);
/* Same, into host memory, as rt_render (w, h and frame_count are accum's). */
int rt_render_adaptive(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                       const rt_filter_cache* filter, uint32_t tile_w, uint32_t tile_h, uint32_t total_frame_index,
                       const rt_adaptive_params* p, rt_accumulation_buffer* accum, uint32_t* out_tile_spp,
                       rt_stats* stats);

/* The robust estimator: a Gini-adaptive median of means (after Buisine, Delepoulle, Renaud, EGSR 2021) over a
 * stack of accumulation buffers, per pixel, in place of the plain mean.  Beyond the reference, whose
 * AccumulationBuffer is a mean: an opt-in of new entries only (no existing struct or entry changes;
 * RT_ABI_VERSION stays).  DESIGN.md ("The robust estimator") defines it operation by operation; the device
 * matches the plain-C restatement tests/ref_robust/ref_robust.c bit for bit.  In short, per pixel:
 *   - the stack is `count` (2..32) buffers of w*h float4 (sum w*rgb, sum w) holding disjoint sample sets of one
 *     frame, buffer k at float offset k*w*h*4 of one allocation;
 *   - buffer k is valid when its weight is > 0.001f, its four floats are finite, m_k = S_k.xyz / S_k.w is
 *     finite and key_k = (m_k.r + m_k.g) + m_k.b is finite; n = the number of valid buffers.  With n = 0 the
 *     pixel is buffer 0's four floats unchanged (the output pass still shows NaN and negative weights);
 *   - the valid buffers are ranked by ascending key (-0 as +0), equal keys by buffer index; their Gini
 *     coefficient G in [0, 1) is taken over max(key, 0) (0 when n < 3 or the keys sum to nothing);
 *   - c = min(floor(gini_scale * G * n/2), (n-1)/2, max_trim) buffers are dropped at each end of the ranking
 *     and the rest pooled: {sum S_k.xyz / sum S_k.w, 1.0f}, added in buffer order.  c = 0 (gini_scale = 0, or
 *     equal buffers) is the pooled mean of the valid buffers;
 *   - info (optional, w*h float4) receives {G, (float)c, (float)n, sum S_k.w of the kept buffers}.
 * The estimate trades energy for variance: it drops the rare bright samples of glass, and with them the part
 * of the true radiance they carry (DESIGN.md has the measurements, losses included). */
typedef struct rt_robust_params {
    uint32_t buffers;      /* K of the drivers: 2..32; default 8 */
    float    gini_scale;   /* >= 0, finite; 0 = pooled mean; default 1.0f */
    uint32_t max_trim;     /* cap of c; default 15 (no cap beyond (n-1)/2) */
    int32_t  reserved[5];
} rt_robust_params;
int    rt_robust_default_params(rt_robust_params* out);                          /* no device needed */
size_t rt_robust_workspace_bytes(uint32_t w, uint32_t h, uint32_t buffers);      /* buffers*w*h*16; no device needed */
/* The stage alone.  d_stack, d_out and d_info (may be NULL) are device pointers on `device`; d_out may be any
 * buffer of the stack (a thread touches only its own pixel).  p->buffers is not read: `count` rules.
 * `hip_stream` may be NULL; returns after the kernel has completed.  RT_ERROR_INVALID by name, before the
 * device is touched: a NULL stack, parameter or output, w or h of 0, a count outside 2..32, a negative or
 * non-finite gini_scale. */
int rt_robust_combine_device(int device, const float* d_stack, uint32_t count, uint32_t w, uint32_t h,
                             const rt_robust_params* p, float* d_out, float* d_info, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_robust_combine(int device, const float* stack, uint32_t count, uint32_t w, uint32_t h,
                      const rt_robust_params* p, float* out, float* info);
/* The driver, written on the public entries.  K = p->buffers; settings->samples_per_pixel must be a positive
 * multiple of K.  The stack (d_workspace: rt_robust_workspace_bytes(w, h, K) bytes; with NULL the call
 * allocates and frees its own) is zeroed; buffer k is shard k of K of the frame by sample passes: rt_render_device
 * with the caller's settings and frame_count, rt_tile_set {tile_w, tile_h, k, K} and the scene's shard mode set to
 * RT_SHARD_PASSES for the call (rt_scene_set_config; put back on every way out), i.e. passes
 * [k*spp/K, (k+1)*spp/K) of every tile.  Together the buffers are exactly the samples a uniform frame of
 * samples_per_pixel draws at frame_count.  (A frame of spp/K samples at frame_count + k*spp/K is not: it takes
 * the same canonical sample indices under other random streams, because a sample's seed hashes its frame's
 * frame_count.)  A pass shard never takes the exact splat: the frames stream, as a rank's share does.  The
 * caller's `tiles` must be unsharded (shard_index 0, shard_count 1).  Then rt_robust_combine_device writes d_out
 * (w*h float4: overwritten, not added to, as the denoise stage's) and d_info (may be NULL).  The counters of
 * `stats` are sums over the frames (those of the uniform frame), `seconds` the wall time of the whole call,
 * splat_mode and shadow_launch the last frame's.  rt_cancel is read after every frame and ends the call with
 * RT_ERROR_CANCELLED (d_out is then untouched).  RT_ERROR_INVALID by name before the device is touched: a NULL
 * parameter, scene, camera, settings, filter, tiles or output; w or h of 0; buffers outside 2..32; a negative or
 * non-finite gini_scale; samples_per_pixel of 0 or no multiple of buffers; sharded tiles.  A frame costs about
 * 2.4 ms whatever it renders, K times here. */
int rt_render_robust_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                            const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                            uint32_t w, uint32_t h, uint32_t frame_count, const rt_robust_params* p,
                            void* d_workspace, float* d_out, float* d_info, void* hip_stream, rt_stats* stats);
/* Same, into host memory (out w*h float4; info w*h float4 or NULL). */
int rt_render_robust(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                     const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                     uint32_t w, uint32_t h, uint32_t frame_count, const rt_robust_params* p, float* out,
                     float* info, rt_stats* stats);
/* rt_render_picture with the robust estimator, written on the public entries: rt_render_robust_device at
 * frame_count 0 into a fresh buffer; with `dp` (may be NULL) the three feature frames of guide_spp samples per
 * pixel (0: settings->samples_per_pixel) by rt_render_features_device and rt_denoise_features_device on the
 * robust output, as rt_render_picture_features_denoised does; rt_postprocess_device with the dither texture
 * of total_frame_index + 1.  `stats` is the driver's. */
int rt_render_picture_robust(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                             const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                             uint32_t w, uint32_t h, const rt_post_settings* post, const rt_robust_params* p,
                             const rt_denoise_features_params* dp, uint32_t guide_spp, uint32_t* out_bgra,
                             rt_stats* stats);

/* Temporal accumulation (beyond the reference, whose main loop resets its back buffer whenever the camera
 * moves, RT/raytracer.cpp:711-720; an opt-in: no other entry calls it).  Two device parts and a driver:
 * a primary-hit G-buffer, a stage that reprojects the previous frame's history through it and blends the
 * current frame in, and one frame of the loop written on the public entries.  DESIGN.md ("Temporal
 * accumulation") defines every operation; both kernels match the plain-C restatement
 * tests/ref_temporal/ref_temporal.c bit for bit.
 *
 * The G-buffer: one closest-hit ray per pixel (x, y), render_tile's camera ray (RT/raytracer.cpp:397-460)
 * without jitter and without the lens offset (a pinhole at camera->p), max_t FLT_MAX, ignored primitive 0.
 * A hit's texel is what rt_debug_intersect(occlusion = 0) returns for that ray: p = hit_p, t, n, primitive
 * (with RT_HIT_PLANE_BIT).  A miss is {p = the ray's direction, t = 0, n = 0, primitive = RT_HIT_MISS}: the
 * sky depends on the direction only, and the stage reprojects it that way. */
typedef struct rt_gbuffer_texel { rt_v3 p; float t; rt_v3 n; uint32_t primitive; } rt_gbuffer_texel;  /* 32 B */
/* d_out: w*h texels on the scene's device.  A fixed grid strides over the pixels; its traversal spill area
 * is allocated with the scene on the first call and freed by rt_scene_free, so later calls allocate nothing.
 * `hip_stream` may be NULL; returns after the kernel has completed.  RT_ERROR_INVALID by name, before the
 * device is touched: a NULL scene, camera or output, w or h of 0, w*h of 2^32 or more. */
int rt_gbuffer_device(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                      rt_gbuffer_texel* d_out, void* hip_stream);
/* Same, into host memory. */
int rt_gbuffer(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
               rt_gbuffer_texel* out);

/* The accumulate stage, one thread per pixel.  In short:
 *   - d_current is an accumulation buffer (sum w*rgb, sum w).  The denoise stage's validity rule applies to
 *     it: weight > 0.001f and a finite resolved colour.  An invalid pixel comes out as it went in (all four
 *     floats) with length 0, and is never used as a tap by the next frame;
 *   - the resolved colour c is clamped to [0, firefly_clamp] per channel (no upper clamp when 0);
 *   - without history (the three d_prev_* pointers NULL: all of them or none) the pixel is {c, 1}, length 1;
 *   - the point P = texel.p of a hit, prev_camera->p + texel.p of a miss, is projected into the previous
 *     camera, prev_lens_distortion is undone by a fixed count of clamped Newton steps (a point beyond the
 *     image's distorted corner radius has no history), and the previous history is read there: the one pixel at the rounded position when both coordinates lie within `snap`
 *     of an integer (a standing camera does not blur its history), the four bilinear taps otherwise;
 *   - a tap counts when it lies in the image, its previous length is >= 1, its history is finite, its
 *     previous texel names the same primitive (as integers) and, for hits, dot(n, n_prev) >= normal_cos and
 *     |dot(p_prev - P, n)| <= plane_tolerance * t;
 *   - with W = the valid taps' weight > 0: hist and L their weighted means, N = min(L + 1, max_history),
 *     out = hist + (c - hist) * (1/N) (c itself when N is 1), length N.  Otherwise {c, 1}, length 1.
 * d_history is w*h float4 {r, g, b, 1}: rt_denoise*_device and rt_postprocess_device take it as it is.
 * d_length is one float per pixel. */
typedef struct rt_temporal_params {
    float   max_history;      /* >= 1; 1 = no history (output is the clamped current frame) */
    float   normal_cos;       /* a tap needs dot(n_cur, n_prev) >= this */
    float   plane_tolerance;  /* and |dot(p_prev - P, n_cur)| <= this * t_cur */
    float   snap;             /* pixels: within this of an integer position, one tap instead of four */
    float   firefly_clamp;    /* as rt_denoise_params; 0 = none */
    int32_t reserved[3];
} rt_temporal_params;
int rt_temporal_default_params(rt_temporal_params* out);      /* 32, 0.9, 0.02, 1/32, 10; no device needed */
/* Device pointers on `device`.  The inputs are only read; d_history and d_length may alias no previous
 * buffer.  `hip_stream` may be NULL; returns after the kernel has completed.  RT_ERROR_INVALID by name,
 * before the device is touched: a NULL d_current, d_gbuffer, parameter, d_history or d_length; some but not
 * all of d_prev_history, d_prev_length and d_prev_gbuffer NULL; a NULL prev_camera with history; w or h of 0;
 * max_history < 1 or non-finite; a negative or non-finite plane_tolerance, snap or firefly_clamp; normal_cos
 * outside [-1, 1]; d_history equal to d_prev_history or d_length to d_prev_length. */
int rt_temporal_accumulate_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                  const float* d_prev_history, const float* d_prev_length,
                                  const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                  float* d_history, float* d_length, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_temporal_accumulate(int device, const float* current, const rt_gbuffer_texel* gbuffer,
                           const float* prev_history, const float* prev_length,
                           const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                           float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                           float* history, float* length);

/* The driver: one frame of an interactive loop, written on the public entries.  `state` is the caller's; all
 * zero means no history.  d_workspace (rt_temporal_workspace_bytes(w, h) bytes on the scene's device: the
 * current frame, then two sets of G-buffer, history and length) is the caller's too and lives as long as the
 * state.  A frame zeroes the current buffer, renders into it with rt_render_device (the caller's settings
 * and frame_count), writes set [parity]'s G-buffer with rt_gbuffer_device (settings->lens_distortion), runs
 * rt_temporal_accumulate_device against set [parity ^ 1] and state->camera (without history when
 * state->frames is 0 or state->w / state->h differ from w / h: the state restarts), copies the history to
 * d_out (w*h float4) and the length to d_length_out (w*h floats; may be NULL), then stores the camera and the
 * lens distortion, flips parity and increments frames.  rt_cancel ends the call with RT_ERROR_CANCELLED and
 * leaves `state` and the outputs as they were.  `stats` is the beauty frame's.  RT_ERROR_INVALID by name
 * before the device is touched: a NULL parameter, state, workspace, settings, camera, filter, tiles, output
 * or scene; w or h of 0; a state's parity above 1; the parameter refusals of the stage. */
size_t rt_temporal_workspace_bytes(uint32_t w, uint32_t h);   /* current 16 + 2 x (32 + 16 + 4) bytes per pixel; no device needed */
typedef struct rt_temporal_state {   /* the caller's; all zero = no history */
    uint32_t  w, h, frames, parity;
    rt_camera camera;
    float     lens_distortion;
    void*     d_workspace;
} rt_temporal_state;
int rt_render_temporal_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                              const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                              uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                              rt_temporal_state* state, float* d_out, float* d_length_out, void* hip_stream,
                              rt_stats* stats);
/* Same, with out_pixels (w*h float4) and out_length (w*h floats; may be NULL) in host memory; the state's
 * workspace stays on the device. */
int rt_render_temporal(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                       const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                       uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                       rt_temporal_state* state, float* out_pixels, float* out_length, rt_stats* stats);

/* Variance-guided filtering of the temporal history (beyond the reference; after Schied et al., "Spatiotemporal
 * Variance-Guided Filtering", HPG 2017, in this project's terms; an opt-in: no other entry calls it, and
 * rt_render_temporal_device is not touched).  Three device parts and a driver: the accumulate stage with the
 * first two moments of the tonemapped luminance beside it, the variance of the history from those moments, an
 * a-trous filter whose colour term is scaled by that variance and whose edge-stopping terms come from the
 * G-buffer (no guide frames), and one frame of the loop written on the public entries.  DESIGN.md
 * ("Variance-guided filtering") defines every operation; the kernels match the plain-C restatement
 * tests/ref_svgf/ref_svgf.c bit for bit.  Throughout, lum(c) = (0.2126 r + 0.7152 g) + 0.0722 b and
 * tm(c) = 1 - expf(-lum(c)), the denoise stage's l, in [0, 1].
 *
 * Accumulate with moments: rt_temporal_accumulate_device's arguments and operations, and d_history and d_length
 * equal to its outputs bit for bit; in addition d_prev_moments (all-or-none with the other three previous
 * buffers) and d_moments, two floats {m1, m2} per pixel (it may not alias d_prev_moments).  An invalid pixel
 * writes {0, 0}.  With t = tm(c) of the clamped current colour: each valid tap also adds wt * m_prev to S1 and S2
 * (the moments take no part in a tap's validity); with W > 0, h = S / W and m = h + ({t, t*t} - h) * (1/N)
 * ({t, t*t} itself when N is 1); without a valid tap or without history {t, t*t}.  The refusals are the
 * accumulate stage's, by name, and a NULL d_moments, a NULL d_prev_moments beside other previous buffers (or
 * the reverse) and d_moments equal to d_prev_moments. */
int rt_temporal_accumulate_moments_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                          const float* d_prev_history, const float* d_prev_length,
                                          const rt_gbuffer_texel* d_prev_gbuffer, const float* d_prev_moments,
                                          const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w,
                                          uint32_t h, const rt_temporal_params* p, float* d_history, float* d_length,
                                          float* d_moments, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_temporal_accumulate_moments(int device, const float* current, const rt_gbuffer_texel* gbuffer,
                                   const float* prev_history, const float* prev_length,
                                   const rt_gbuffer_texel* prev_gbuffer, const float* prev_moments,
                                   const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                   const rt_temporal_params* p, float* history, float* length, float* moments);

/* The variance of the history, one float per pixel: the variance of the mean that the history holds, so a long
 * history filters less.  A pixel whose length is not >= 1 gets 0.  With length >= spatial_below,
 * s2 = max(m2 - m1*m1, 0).  Otherwise the moments are averaged over a 7x7 window of the current frame: a
 * neighbour counts when it lies in the image, its length is >= 1 and it is the same surface by the accumulate
 * stage's rule within this frame's G-buffer (the same primitive and, for hits, dot(n_p, n_q) >= p->normal_cos
 * and |dot(p_q - p_p, n_p)| <= p->plane_tolerance * t_p); the centre always counts; s2 from the window's means.
 * The output is s2 / length.  Of `p` only normal_cos and plane_tolerance are used, and all of it is checked.
 * RT_ERROR_INVALID by name before the device is touched: a NULL pointer, w or h of 0, the parameter refusals
 * of the accumulate stage, a negative or non-finite spatial_below, d_variance equal to an input. */
#define RT_TEMPORAL_SPATIAL_BELOW_DEFAULT 4.0f
int rt_temporal_variance_device(int device, const float* d_moments, const float* d_length,
                                const rt_gbuffer_texel* d_gbuffer, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                float spatial_below, float* d_variance, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_temporal_variance(int device, const float* moments, const float* length, const rt_gbuffer_texel* gbuffer,
                         uint32_t w, uint32_t h, const rt_temporal_params* p, float spatial_below, float* variance);

/* The variance-guided filter.  d_color is w*h float4, resolved and clamped as the denoise stage resolves beauty
 * (a history {r, g, b, 1} passes as it is); d_variance one float per pixel; d_gbuffer the frame's texels.  A
 * pixel is valid by the denoise stage's rule on the colour and when its variance is >= 0 and finite; invalid
 * pixels come out as they went in (all four floats, and their variance) and contribute to no neighbour.
 * Iteration i (step 2^i) of `iterations`, for a valid pixel p: gv = the 3x3 Gaussian {1/16, 1/8, 1/4} of the
 * current variance over the valid neighbours at distance 1; the 5x5 B3-spline kernel with holes of the denoise
 * stage, skipping taps outside the image, invalid taps and taps where exactly one of p and q is a miss; each
 * tap weighted by expf(-e), e = |l(p) - l(q)| / (sigma_color sqrt(gv) + variance_epsilon)
 * + |n_p - n_q|^2 / sigma_normal^2 + (dot(p_q - p_p, n_p) / t_p)^2 / sigma_plane^2 (the last two for a hit p
 * only; l = tm of the current colour); c' = sum(wt c) / sum(wt), var' = sum(wt^2 var) / sum(wt)^2.  A valid pixel
 * comes out as {r, g, b, 1.0f}, so rt_postprocess_device takes the buffer as it is. */
typedef struct rt_denoise_variance_params {
    int32_t iterations;        /* 1..8 */
    float   sigma_color;       /* in standard deviations of the tonemapped luminance; 0 = term off */
    float   sigma_normal;      /* on the raw normals' difference; 0 = term off */
    float   sigma_plane;       /* on the offset along p's normal over p's distance; 0 = term off */
    float   variance_epsilon;  /* > 0: the colour term's floor where the variance is 0 */
    float   firefly_clamp;     /* as rt_denoise_params; 0 = none */
    int32_t reserved[2];
} rt_denoise_variance_params;
int    rt_denoise_variance_default_params(rt_denoise_variance_params* out);   /* 4, 4, 0.2, 0.02, 0.03, 10; no device needed */
size_t rt_denoise_variance_workspace_bytes(uint32_t w, uint32_t h);           /* 40 bytes per pixel; no device needed */
/* Device pointers on `device`; d_out (w*h float4) may equal d_color, d_variance_out (w*h floats; may be NULL)
 * may equal d_variance.  d_workspace holds rt_denoise_variance_workspace_bytes(w, h) bytes; with NULL the call
 * allocates and frees its own.  `hip_stream` may be NULL; returns after the filter has completed.
 * RT_ERROR_INVALID by name before the device is touched: a NULL d_color, d_variance, d_gbuffer, parameter or
 * d_out; w or h of 0; iterations outside 1..8; a negative or non-finite sigma or clamp; a variance_epsilon that
 * is not finite and > 0; d_out equal to d_variance or d_gbuffer; d_variance_out equal to d_color, d_gbuffer or
 * d_out; w or h above 65535; a d_gbuffer or d_workspace that is not 16-byte aligned. */
int rt_denoise_variance_device(int device, const float* d_color, const float* d_variance,
                               const rt_gbuffer_texel* d_gbuffer, uint32_t w, uint32_t h,
                               const rt_denoise_variance_params* p, void* d_workspace, float* d_out,
                               float* d_variance_out, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_denoise_variance(int device, const float* color, const float* variance, const rt_gbuffer_texel* gbuffer,
                        uint32_t w, uint32_t h, const rt_denoise_variance_params* p, float* out, float* variance_out);

/* The driver: one frame of the interactive loop with the filter, written on the public entries.  `state` is the
 * caller's, all zero means no history; d_workspace (rt_temporal_filtered_workspace_bytes(w, h) bytes on the
 * scene's device, 16-byte aligned) is the caller's too and lives as long as the state.  A frame zeroes the
 * current buffer, renders into it with rt_render_device, writes set [parity]'s G-buffer with rt_gbuffer_device,
 * runs rt_temporal_accumulate_moments_device against set [parity ^ 1] and state->camera (without history when
 * state->frames is 0 or the frame size changed: the state restarts), rt_temporal_variance_device on the new
 * set, and rt_denoise_variance_device from the new history into d_out (w*h float4).  The history that the
 * next frame reads stays the unfiltered one.  The optional outputs (each may be NULL) are that unfiltered
 * history (w*h float4), its length and the variance the filter was given (w*h floats each).  Then the camera
 * and the lens distortion are stored, parity flips and frames increments.  rt_cancel ends the call with
 * RT_ERROR_CANCELLED and leaves `state` and the outputs as they were.  `stats` is the beauty frame's.
 * RT_ERROR_INVALID by name before the device is touched, in rt_render_temporal_device's order: the parameter
 * refusals of the three stages, then a NULL state, workspace, settings, camera, filter, tiles, output or scene,
 * w or h of 0, a parity above 1. */
size_t rt_temporal_filtered_workspace_bytes(uint32_t w, uint32_t h);   /* 180 bytes per pixel; no device needed */
typedef struct rt_temporal_filtered_state {   /* the caller's; all zero = no history */
    uint32_t  w, h, frames, parity;
    rt_camera camera;
    float     lens_distortion;
    void*     d_workspace;
} rt_temporal_filtered_state;
int rt_render_temporal_filtered_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                       const rt_filter_cache* filter, const rt_tile_set* tiles,
                                       uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                       const rt_temporal_params* p, float spatial_below,
                                       const rt_denoise_variance_params* fp, rt_temporal_filtered_state* state,
                                       float* d_out, float* d_history_out, float* d_length_out, float* d_variance_out,
                                       void* hip_stream, rt_stats* stats);
/* Same, with the four outputs in host memory (all but out_pixels may be NULL); the state's workspace stays on the
 * device. */
int rt_render_temporal_filtered(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                                uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                                float spatial_below, const rt_denoise_variance_params* fp,
                                rt_temporal_filtered_state* state, float* out_pixels, float* out_history,
                                float* out_length, float* out_variance, rt_stats* stats);

/* Moving instances after upload, and a history that follows them (beyond the reference, an opt-in: new entries
 * only, no other entry changes; RT_ABI_VERSION stays).  DESIGN.md ("Moving instances") defines the update and the
 * stage operation by operation; the stage's kernel matches tests/ref_motion/ref_motion.c bit for bit.
 *
 * rt_scene_update_instances replaces the transform-dependent tables of an uploaded scene: the transforms, the
 * top-level BVH with its prologue sequences and leaf records, and the small-table blob.  `desc` must describe the
 * uploaded scene except for transforms[] (whose count may change), primitives[i].transform_index and the top-level
 * BVH (bvh_nodes, bvh_indices and their counts).  The counts of materials, primitives, planes, lights and meshes
 * and each primitive's type, material_id, mesh_index and p[] must equal the uploaded ones (planes and lights are
 * compared whole): a mismatch is RT_ERROR_INVALID by name.  desc->materials, desc->skydome and the meshes'
 * triangles / normals / nodes / indices are never read and may be NULL: no mesh, sky or material byte is uploaded
 * again.  Every check (index ranges, the BVH's depth against the 64-entry traversal stack, traversal_ref's bound)
 * happens before the device is touched: a refused update leaves the scene exactly as it was.  The entry
 * synchronises the device before it replaces a table.  After it every entry on the scene is bit-identical to the
 * same entry on a fresh rt_scene_upload of `desc`; the scene's config, recursive opt-in, ambient light,
 * partitions and spill areas survive. */
int rt_scene_update_instances(rt_scene* scene, const rt_scene_desc* desc);
/* The resolved transform of every primitive (transforms[primitives[i].transform_index]) as of the upload or the
 * last update, from a host copy: out[0 .. min(cap, count)) and *out_count = the scene's primitive count.  out may
 * be NULL with cap 0.  No device work. */
int rt_scene_primitive_transforms(const rt_scene* scene, uint32_t cap, rt_m4x4inv* out, uint32_t* out_count);

/* One primitive's rigid motion between two frames: a world point P of the current frame lies at
 * fwd_prev * (inv_cur * P) in the previous one (rows 0..2 of the current inverse and of the previous forward). */
typedef struct rt_motion_entry {   /* 112 B */
    float    inv_cur[3][4];
    float    fwd_prev[3][4];
    uint32_t moved;                /* 1: any of the 24 words of forward rows 0..2 and inverse rows 0..2 differs */
    uint32_t reserved[3];          /* 0 */
} rt_motion_entry;
/* out[i] from cur[i] and prev[i], i < count; the words are compared as integers.  No device needed. */
int rt_motion_table(uint32_t count, const rt_m4x4inv* cur, const rt_m4x4inv* prev, rt_motion_entry* out);

/* The motion-aware accumulate stage: rt_temporal_accumulate_device's arguments and operations with one new step.
 * For a hit whose primitive has no RT_HIT_PLANE_BIT, is below motion_count and whose entry has moved != 0:
 *   Po.k = ((a[k][0]*P.x + a[k][1]*P.y) + a[k][2]*P.z) + a[k][3], a = inv_cur;  Q likewise from Po with fwd_prev;
 *   m likewise from n through the two 3 x 3 parts (no translation), divided by its length when that is > 0 (else
 *   m = n);
 * and Q and m stand where P and n stand in the projection and in the tap tests; plane_limit stays
 * plane_tolerance * t.  Every other pixel (a miss, a plane, an id >= motion_count, moved == 0, d_motion NULL) takes
 * rt_temporal_accumulate_device's path word for word.  d_motion NULL requires motion_count 0.
 * d_moments (w*h float2, optional) receives rt_temporal_accumulate_moments_device's moments; with it and a history
 * d_prev_moments is required, without it d_prev_moments must be NULL.  d_velocity (w*h float2, optional) receives
 * (fx - x, fy - y) where the projection into the previous frame succeeds and two quiet NaNs (0x7FC00000) elsewhere:
 * invalid current pixels and calls without history among them. */
int rt_temporal_accumulate_motion_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                         const float* d_prev_history, const float* d_prev_length,
                                         const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                         float prev_lens_distortion, uint32_t w, uint32_t h,
                                         const rt_temporal_params* p, float* d_history, float* d_length,
                                         void* hip_stream, const rt_motion_entry* d_motion, uint32_t motion_count,
                                         const float* d_prev_moments, float* d_moments, float* d_velocity);
/* Same on host buffers (motion: motion_count entries on the host). */
int rt_temporal_accumulate_motion(int device, const float* current, const rt_gbuffer_texel* gbuffer,
                                  const float* prev_history, const float* prev_length,
                                  const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                  float* history, float* length, const rt_motion_entry* motion,
                                  uint32_t motion_count, const float* prev_moments, float* moments, float* velocity);

/* The driver: rt_render_temporal_device's frame with the motion-aware stage, written on the public entries.
 * `state` is the caller's, all zero but its three pointers at the start: d_workspace
 * (rt_temporal_motion_workspace_bytes(w, h, the scene's primitive count) bytes on the scene's device:
 * rt_temporal_workspace_bytes(w, h), then the table) and transforms, a host array of transform_cap entries
 * (>= the scene's primitive count).  A frame renders into the workspace and writes the G-buffer as
 * rt_render_temporal_device does, takes the current transforms with rt_scene_primitive_transforms, builds the
 * table with rt_motion_table against state->transforms and uploads it, runs
 * rt_temporal_accumulate_motion_device (without history when state->frames is 0, the frame size changed or
 * state->primitive_count differs from the scene's: the state restarts), copies the history (and the length)
 * out, and stores the camera and the transforms in the state.  rt_cancel and the refusals are
 * rt_render_temporal_device's, plus a NULL transforms or a transform_cap below the scene's primitive count. */
size_t rt_temporal_motion_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count);   /* no device needed */
typedef struct rt_temporal_motion_state {   /* the caller's */
    uint32_t   w, h, frames, parity;
    rt_camera  camera;
    float      lens_distortion;
    uint32_t   primitive_count;             /* of the stored transforms */
    uint32_t   transform_cap;               /* entries `transforms` has room for */
    void*      d_workspace;
    rt_m4x4inv* transforms;                 /* host */
} rt_temporal_motion_state;
int rt_render_temporal_motion_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                     const rt_filter_cache* filter, const rt_tile_set* tiles,
                                     uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                     const rt_temporal_params* p, rt_temporal_motion_state* state, float* d_out,
                                     float* d_length_out, void* hip_stream, rt_stats* stats);
int rt_render_temporal_motion(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                              const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                              uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                              rt_temporal_motion_state* state, float* out_pixels, float* out_length,
                              rt_stats* stats);

/* Deforming meshes after upload (beyond the reference, an opt-in: new entries only, no other entry's behaviour
 * changes; RT_ABI_VERSION stays).  DESIGN.md ("Deforming meshes") defines the refit operation by operation; the
 * kernels match tests/ref_refit/ref_refit.c and rth_update_mesh byte for byte.
 *
 * rt_scene_update_mesh_device gives mesh `mesh_index` of an uploaded scene new vertices.  d_triangles (on the scene's
 * device) holds 9 floats per triangle, a b c, in the ORIGINAL order: the order rth_create_mesh took them in, which
 * is rt_mesh::normals' order and what rt_mesh::indices maps a BVH slot to.  d_normals holds 3 x 3 floats per triangle
 * in the same order, or is NULL: the stored normals stay.  The mesh's topology stays: left_first, count, split_axis,
 * the slot order and the BVH4's records.  Rewritten, for this mesh only: its triangle records, its slot-order
 * normals, the box of every node reachable from node 0 that has a triangle below it (in both node tables), the
 * child boxes of its BVH4 nodes and their skipped-level boxes.  out_root (optional) receives node 0 afterwards.
 * Refused with RT_ERROR_INVALID, by name, before any table changes: a null scene, a mesh_index out of range, null
 * triangles for a mesh that has some, normals for a mesh uploaded without, a vertex that is not finite or a triangle
 * whose box is not within 2^40 of the origin (a reduction on the device; its flag comes back in one small copy), a
 * mesh BVH that is no tree.  A refused call leaves every table's bytes as they were.  The entry synchronises the
 * device first and is complete on return.
 * When node 0's box changed, the scene is stale: its instance tables and the caller's top-level BVH still hold the
 * old box.  Until a successful rt_scene_update_instances (with a top-level BVH over the new bounds) every entry that
 * traces rays through the scene returns RT_ERROR_INVALID and says so.  An update that leaves the root box's bytes as
 * they were does not make the scene stale.  After update + rt_scene_update_instances every entry on the scene is
 * bit-identical to the same entry on a fresh rt_scene_upload of the rth_update_mesh-ed host scene. */
int rt_scene_update_mesh_device(rt_scene* scene, uint32_t mesh_index, const float* d_triangles, const float* d_normals,
                                rt_bvh_node* out_root);
/* Same, with triangles and normals in host memory. */
int rt_scene_update_mesh(rt_scene* scene, uint32_t mesh_index, const float* triangles, const float* normals,
                         rt_bvh_node* out_root);
/* For the tests: one mesh's slice of a scene table, copied to `out` (cap bytes); *out_bytes = the slice's size.  out
 * NULL asks for the size alone; a cap below it is RT_ERROR_INVALID.  The two plan tables build the mesh's refit plan
 * when no update has yet. */
enum rt_mesh_table {
    RT_MESH_TABLE_TRIANGLES    = 0,   /* 12 floats per slot: (a, 0), (b - a, 0), (c - a, 0)                  */
    RT_MESH_TABLE_NORMALS      = 1,   /* 9 floats per slot                                                   */
    RT_MESH_TABLE_NODES_SRC    = 2,   /* rt_bvh_node per node, the caller's layout                           */
    RT_MESH_TABLE_NODES        = 3,   /* the traversal layout: the same boxes, the packed record, 0          */
    RT_MESH_TABLE_NODES4       = 4,   /* 32 floats per BVH4 node (rt_debug_mesh_bvh4's layout)               */
    RT_MESH_TABLE_MID4         = 5,   /* 12 floats per BVH4 node: pL rL pR rR of its BVH2 node's children    */
    RT_MESH_TABLE_BVH4_SOURCES = 6,   /* uint32 per BVH4 node: the BVH2 node it was made from                */
    /* 8 uint32: launches of the subtree kernel (rounds), subtrees, subtrees of the first round, nodes reachable from
     * node 0, the largest subtree's nodes, the most levels in one subtree, BVH4 nodes, kernel launches per update */
    RT_MESH_TABLE_REFIT_PLAN   = 7,
    RT_MESH_TABLE_COUNT        = 8
};
int rt_debug_scene_mesh_table(const rt_scene* scene, uint32_t mesh_index, int which, void* out, size_t cap,
                              size_t* out_bytes);

/* A temporal history that follows deforming meshes (beyond the reference, an opt-in: new entries only, no other
 * entry's behaviour changes; RT_ABI_VERSION stays).  DESIGN.md ("Deforming meshes keep their history") defines the
 * stage operation by operation; its kernel matches tests/ref_deform/ref_deform.c bit for bit.
 *
 * The surface record: beside each G-buffer texel, which triangle the primary hit lies on and where.  For a hit on a
 * mesh primitive `triangle` is the mesh-local ORIGINAL index (the order of rt_mesh::normals and of
 * rt_scene_update_mesh_device's input) and v, w are the hit's barycentrics, the floats the shading normal is
 * interpolated with (u = 1 - v - w belongs to the triangle's first vertex).  Every other pixel (a miss, a plane, a
 * sphere, a box) holds {0xFFFFFFFF, 0, 0, 0}. */
typedef struct rt_surface_texel { uint32_t triangle; float v, w; uint32_t reserved; } rt_surface_texel;  /* 16 B */
/* rt_gbuffer_device with the record: d_out receives rt_gbuffer_device's texels bit for bit, d_surface w*h records.
 * The same fixed grid, spill area and refusals, plus a NULL d_surface. */
int rt_gbuffer_surface_device(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                              rt_gbuffer_texel* d_out, rt_surface_texel* d_surface, void* hip_stream);
/* Same, into host memory. */
int rt_gbuffer_surface(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                       rt_gbuffer_texel* out, rt_surface_texel* surface);

/* The deform table.  A caller lists, per frame, the meshes it deformed since the previous frame, each with the
 * vertex buffer (and normals) the PREVIOUS frame was rendered with: the arrays it gave the update before the last
 * one (or the upload's, in original order), still on the scene's device.  The caller double-buffers. */
typedef struct rt_deform_mesh {
    uint32_t     mesh_index, reserved;
    const float* d_prev_triangles;     /* 9 floats a triangle, original order, on the scene's device */
    const float* d_prev_normals;       /* 9 floats a triangle, or NULL for a mesh uploaded without normals */
} rt_deform_mesh;
typedef struct rt_deform_entry {       /* 128 B, one per primitive */
    float        inv_prev[3][4], fwd_prev[3][4];    /* rows 0..2 of the previous frame's inverse and forward */
    const float* d_prev_triangles;
    const float* d_prev_normals;
    uint32_t     triangle_count, deformed, has_normals, reserved;
} rt_deform_entry;
/* out[i], i < primitive_count, from prev[i] (what rt_scene_primitive_transforms returned the frame before).  A mesh
 * primitive whose mesh_index is listed takes deformed = 1, the two pointers, the mesh's triangle count and
 * has_normals from the scene's host copies; every other entry has deformed = 0, NULL pointers and 0 counts.  Host
 * only, no device work.  RT_ERROR_INVALID by name: a NULL scene, NULL meshes with a mesh_count, NULL prev or out with
 * a primitive_count, a primitive_count other than the scene's, a mesh_index out of range or listed twice, NULL
 * d_prev_triangles, NULL d_prev_normals for a mesh uploaded with normals or non-NULL for one without. */
int rt_scene_deform_table(const rt_scene* scene, uint32_t mesh_count, const rt_deform_mesh* meshes,
                          uint32_t primitive_count, const rt_m4x4inv* prev, rt_deform_entry* out);

/* The deform-aware accumulate stage: rt_temporal_accumulate_motion_device's arguments and operations with one more
 * case, taken before the motion case.  For a hit without RT_HIT_PLANE_BIT whose primitive is below deform_count, whose
 * entry e has deformed != 0 and whose surface record has triangle < e.triangle_count, with a', b', c' the nine floats
 * at e.d_prev_triangles + 9*triangle:
 *   e1 = b' - a';  e2 = c' - a';  Po.k = (a'.k + v*e1.k) + w*e2.k
 *   Q.k = ((f[k][0]*Po.x + f[k][1]*Po.y) + f[k][2]*Po.z) + f[k][3],  f = fwd_prev
 *   no = has_normals ? (u*n0 + v*n1) + w*n2 with u = 1 - v - w and n0..n2 at e.d_prev_normals + 9*triangle
 *                    : cross(normalize(e1), normalize(e2))
 *   n' = the shading normal of `no` under inv_prev (the renderer's transform_normal, then its normalize-or-zero)
 * and Q and n' stand where P and the texel's n stand in the projection and in the tap tests: they are the p and n
 * the previous G-buffer held for this surface point.  plane_limit stays plane_tolerance * t.  Every other pixel
 * takes rt_temporal_accumulate_motion_device's path word for word.  d_deform NULL requires deform_count 0 and allows a
 * NULL d_surface; a table requires d_surface.  The other refusals are the motion stage's. */
int rt_temporal_accumulate_deform_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                         const float* d_prev_history, const float* d_prev_length,
                                         const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                         float prev_lens_distortion, uint32_t w, uint32_t h,
                                         const rt_temporal_params* p, float* d_history, float* d_length,
                                         void* hip_stream, const rt_motion_entry* d_motion, uint32_t motion_count,
                                         const float* d_prev_moments, float* d_moments, float* d_velocity,
                                         const rt_surface_texel* d_surface, const rt_deform_entry* d_deform,
                                         uint32_t deform_count);
/* Same on host buffers; the table's entries are on the host, the vertex pointers inside them stay device pointers. */
int rt_temporal_accumulate_deform(int device, const float* current, const rt_gbuffer_texel* gbuffer,
                                  const float* prev_history, const float* prev_length,
                                  const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                  float* history, float* length, const rt_motion_entry* motion,
                                  uint32_t motion_count, const float* prev_moments, float* moments, float* velocity,
                                  const rt_surface_texel* surface, const rt_deform_entry* deform,
                                  uint32_t deform_count);

/* The driver: rt_render_temporal_motion_device's frame, state and arguments with rt_gbuffer_surface_device in place
 * of rt_gbuffer_device, rt_scene_deform_table against state->transforms beside rt_motion_table, and the deform stage
 * in place of the motion stage.  The workspace is rt_temporal_motion_workspace_bytes, then one surface buffer of 16 B
 * a pixel, then the deform table of 128 B a primitive.  `meshes` lists what deformed since the previous frame, with
 * the buffers the previous frame's update was given; the list is checked on every frame, also on one that runs
 * without history.  A frame's order for the caller: rt_scene_update_mesh_device with the new vertices, the top-level
 * BVH and rt_scene_update_instances, then this driver. */
size_t rt_temporal_deform_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count);   /* no device needed */
int rt_render_temporal_deform_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                     const rt_filter_cache* filter, const rt_tile_set* tiles,
                                     uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                     const rt_temporal_params* p, rt_temporal_motion_state* state,
                                     uint32_t mesh_count, const rt_deform_mesh* meshes, float* d_out,
                                     float* d_length_out, void* hip_stream, rt_stats* stats);
int rt_render_temporal_deform(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                              const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                              uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                              rt_temporal_motion_state* state, uint32_t mesh_count, const rt_deform_mesh* meshes,
                              float* out_pixels, float* out_length, rt_stats* stats);

/* Neighbourhood clipping of the temporal history against ghosting (beyond the reference, an opt-in: new entries only,
 * no other entry's behaviour changes; RT_ABI_VERSION stays).  Variance clipping after Salvi, "An excursion in temporal
 * supersampling" (GDC 2016), in this project's terms.  DESIGN.md ("Neighbourhood clipping") defines both stages
 * operation by operation; the kernels match tests/ref_clip/ref_clip.c bit for bit.
 *
 * The statistics of the current frame: per pixel, the mean and the standard deviation of the resolved colours in the
 * (2 radius + 1)^2 window around it.  A pixel's value is the accumulate stage's steps 1 and 2: valid when its weight
 * is above 0.001f and its resolved colour is finite, clamped per channel to [0, firefly_clamp] (no upper clamp when
 * firefly_clamp is 0).  An invalid pixel and a pixel outside the image add +0 to all seven sums: the three channels,
 * their squares and a count of 1.0f per valid pixel.  Each sum is taken in the separable order: a row sum
 * H(x, y') = ((v(x-r) + v(x-r+1)) + ...) + v(x+r) for y' = y-r .. y+r, then S = ((H(x, y-r) + H(x, y-r+1)) + ...) + H(x, y+r).
 * With n = count > 0: mean = S1/n, var = S2/n - mean*mean, var = var > 0 ? var : 0 (a NaN goes to 0), sigma =
 * sqrtf(var); with n = 0 the texel is all zero.  A texel is written for every pixel, invalid centres included;
 * reserved is 0.  RT_ERROR_INVALID by name before the device is touched: a NULL buffer, w or h of 0, w*h of 2^32 or
 * more, a radius outside 1..3, a negative or non-finite firefly_clamp, d_out equal to d_current. */
typedef struct rt_neighbourhood_texel { rt_v3 mean; float count; rt_v3 sigma; float reserved; } rt_neighbourhood_texel;  /* 32 B */
int rt_temporal_neighbourhood_device(int device, const float* d_current, uint32_t w, uint32_t h, uint32_t radius,
                                     float firefly_clamp, rt_neighbourhood_texel* d_out, void* hip_stream);
/* Same, from and to host memory.  RT_ERROR_NO_DEVICE without a GPU (after the argument checks). */
int rt_temporal_neighbourhood(int device, const float* current, uint32_t w, uint32_t h, uint32_t radius,
                              float firefly_clamp, rt_neighbourhood_texel* out);

/* The accumulate stage with a clip: rt_temporal_accumulate_deform_device's arguments and operations with one more
 * step, 4c, between the taps and the blend.  It runs when d_neighbourhood is non-NULL, the taps' weight W is above 0
 * and the pixel's texel has count >= min_count.  With hist = sum / W, per channel k:
 *   lo = mean_k - gamma*sigma_k;  hi = mean_k + gamma*sigma_k
 *   hist_k = hist_k < lo ? lo : hist_k;  then hist_k = hist_k > hi ? hi : hist_k      (a NaN bound leaves it alone)
 * and the blend runs on the clipped hist.  d_clip_amount (w*h floats, optional) receives the largest of the three
 * |before - after|, and 0 for a pixel that was not clipped, had no history or is invalid.  Length, moments and
 * velocity are the deform stage's bit for bit: the clip does not touch them.  With d_neighbourhood NULL every output is
 * rt_temporal_accumulate_deform_device's.  The refusals are the deform stage's, plus a negative or non-finite gamma or
 * min_count. */
typedef struct rt_temporal_clip_params {
    uint32_t radius;       /* of the statistics' window, 1..3 */
    float    gamma;        /* the box's half width in standard deviations */
    float    min_count;    /* a texel with fewer valid window pixels does not clip */
    uint32_t reserved;
} rt_temporal_clip_params;
int rt_temporal_clip_default_params(rt_temporal_clip_params* out);   /* 3, 0.5, 2; no device needed */
int rt_temporal_accumulate_clip_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                       const float* d_prev_history, const float* d_prev_length,
                                       const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                       float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                       float* d_history, float* d_length, void* hip_stream,
                                       const rt_motion_entry* d_motion, uint32_t motion_count,
                                       const float* d_prev_moments, float* d_moments, float* d_velocity,
                                       const rt_surface_texel* d_surface, const rt_deform_entry* d_deform,
                                       uint32_t deform_count, const rt_neighbourhood_texel* d_neighbourhood, float gamma,
                                       float min_count, float* d_clip_amount);
/* Same on host buffers; the deform table's vertex pointers stay device pointers. */
int rt_temporal_accumulate_clip(int device, const float* current, const rt_gbuffer_texel* gbuffer,
                                const float* prev_history, const float* prev_length,
                                const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                float* history, float* length, const rt_motion_entry* motion, uint32_t motion_count,
                                const float* prev_moments, float* moments, float* velocity,
                                const rt_surface_texel* surface, const rt_deform_entry* deform, uint32_t deform_count,
                                const rt_neighbourhood_texel* neighbourhood, float gamma, float min_count,
                                float* clip_amount);

/* The driver: rt_render_temporal_deform_device's frame, state and arguments with the clip.  A frame renders the
 * current frame, writes the surface G-buffer, runs rt_temporal_neighbourhood_device on the current frame
 * (cp->radius, p->firefly_clamp), builds and uploads the motion and deform tables, runs
 * rt_temporal_accumulate_clip_device (cp->gamma, cp->min_count), copies the history, the length and the clip amounts
 * (d_clip_amount_out, w*h floats; may be NULL) out and advances the state.  mesh_count 0 is the motion loop, unchanged
 * transforms the plain one.  The workspace is rt_temporal_deform_workspace_bytes, then the neighbourhood texels on a
 * 16-byte boundary (32 B a pixel), then the clip amounts (4 B a pixel).  rt_cancel and the refusals are the deform
 * driver's, plus a NULL rt_temporal_clip_params, a radius outside 1..3 and a negative or non-finite gamma or
 * min_count. */
size_t rt_temporal_clipped_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count);   /* no device needed */
int rt_render_temporal_clipped_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                      const rt_filter_cache* filter, const rt_tile_set* tiles,
                                      uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                      const rt_temporal_params* p, rt_temporal_motion_state* state,
                                      uint32_t mesh_count, const rt_deform_mesh* meshes,
                                      const rt_temporal_clip_params* cp, float* d_out, float* d_length_out,
                                      float* d_clip_amount_out, void* hip_stream, rt_stats* stats);
int rt_render_temporal_clipped(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                               const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                               uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                               rt_temporal_motion_state* state, uint32_t mesh_count, const rt_deform_mesh* meshes,
                               const rt_temporal_clip_params* cp, float* out_pixels, float* out_length,
                               float* out_clip_amount, rt_stats* stats);

/* A specular G-buffer: a G-buffer that follows the camera ray through mirrors and glass (beyond the reference, an
 * opt-in: new entries only, no other entry's behaviour changes; RT_ABI_VERSION stays).  DESIGN.md ("A specular
 * G-buffer") defines the walk operation by operation; the kernel matches tests/ref_specular/ref_specular.c bit for bit.
 *
 * The camera ray is rt_gbuffer_device's.  At every hit the walk takes the majority lobe of the feature frames' vertex
 * without a draw: it reflects perfectly where the Fresnel term (1 for total internal reflection, raised by
 * `metallic`) is at least reflect_threshold, else refracts into a participating medium, else ends.  It carries the
 * path length T, the product M of the reflections' Householder matrices and a material stack of 8 levels.  The texel of
 * a walk that took no event is rt_gbuffer_device's bit for bit.  After events and a final hit it is the unfolded
 * point: p = camera.p + T*D (D the camera ray's direction), t = T, n = M*N of the final hit, primitive the final
 * hit's; after events and a miss it is {D, 0, 0, RT_HIT_MISS}.  For planar mirrors p is the mirror image of the
 * surface seen, fixed in world space, so the temporal stages reproject it as they stand; through refraction it is an
 * approximation their plane tolerance judges.
 *
 * The side record (d_chain, optional): the camera ray's own hit (first_primitive, first_t; RT_HIT_MISS and 0 on a
 * miss), chain = the events taken in bits 0..7 and bit 8 + k set when event k was a reflection, end = why the walk
 * ended.  No stage reads it.
 *
 * RT_ERROR_INVALID by name before any launch: rt_gbuffer_device's refusals, a NULL params, max_events above 16, a
 * negative or non-finite reflect_threshold or roughness_max, a scene that awaits rt_scene_update_instances after
 * rt_scene_update_mesh changed a mesh's bounds. */
enum rt_specular_end {
    RT_SPECULAR_END_MISS    = 0,   /* the last ray left the scene */
    RT_SPECULAR_END_EMITTER = 1,   /* the material on the far side of the hit is emissive */
    RT_SPECULAR_END_DIFFUSE = 2,   /* neither lobe was specular: the diffuse branch */
    RT_SPECULAR_END_ROUGH   = 3,   /* a reflection off a material rougher than roughness_max */
    RT_SPECULAR_END_STACK   = 4,   /* a refraction into a medium with the stack's 8 levels in use */
    RT_SPECULAR_END_CAP     = 5    /* another event would pass max_events */
};
typedef struct rt_specular_texel2 { uint32_t first_primitive; float first_t; uint32_t chain, end; } rt_specular_texel2;  /* 16 B */
typedef struct rt_gbuffer_specular_params {
    uint32_t max_events;           /* 0..16; 0 is rt_gbuffer_device */
    float    reflect_threshold;    /* a vertex reflects when its reflectance is at least this */
    float    roughness_max;        /* a reflecting material rougher than this ends the walk as a surface */
    uint32_t reserved;
} rt_gbuffer_specular_params;
int rt_gbuffer_specular_default_params(rt_gbuffer_specular_params* out);   /* 8, 0.5, 0.25; no device needed */
int rt_gbuffer_specular_device(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                               const rt_gbuffer_specular_params* params, rt_gbuffer_texel* d_out,
                               rt_specular_texel2* d_chain, void* hip_stream);
/* Same, into host memory (chain may be NULL). */
int rt_gbuffer_specular(rt_scene* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                        const rt_gbuffer_specular_params* params, rt_gbuffer_texel* out, rt_specular_texel2* chain);

/* The driver: one frame of rt_render_temporal_device's loop over an rt_temporal_state with the specular G-buffer in
 * rt_gbuffer_device's place.  cp NULL: the accumulate stage is rt_temporal_accumulate_device.  Otherwise the frame also
 * runs rt_temporal_neighbourhood_device (cp->radius, p->firefly_clamp) and accumulates with
 * rt_temporal_accumulate_clip_device (cp->gamma, cp->min_count) without motion, deform or surface tables.  The
 * workspace is rt_temporal_workspace_bytes, then the neighbourhood texels on a 16-byte boundary (32 B a pixel).  A
 * virtual point follows no motion or deform table: moved instances and deformed meshes are for the other drivers.
 * rt_cancel, the restart rules and the refusals are rt_render_temporal_device's, plus the G-buffer's and, with a cp,
 * the clipped driver's for it. */
size_t rt_temporal_specular_workspace_bytes(uint32_t w, uint32_t h);   /* no device needed */
int rt_render_temporal_specular_device(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                       const rt_filter_cache* filter, const rt_tile_set* tiles,
                                       uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                       const rt_temporal_params* p, rt_temporal_state* state,
                                       const rt_gbuffer_specular_params* sp, const rt_temporal_clip_params* cp,
                                       float* d_out, float* d_length_out, void* hip_stream, rt_stats* stats);
int rt_render_temporal_specular(rt_scene* scene, const rt_camera* camera, const rt_settings* settings,
                                const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                                uint32_t w, uint32_t h, uint32_t frame_count, const rt_temporal_params* p,
                                rt_temporal_state* state, const rt_gbuffer_specular_params* sp,
                                const rt_temporal_clip_params* cp, float* out_pixels, float* out_length, rt_stats* stats);

/* The reference's top-down BVH builders on the device (RT/bvh.cpp:222-326 with
 * partition_midpoint :53-61, partition_sah_binned :138-213 or the full SAH sweep
 * partition_objects_sah / evaluate_sah :63-131, the partition of :26-51): one launch per
 * tree level and one workgroup per node; the full sweep runs three launches per level and
 * spreads each node's candidate splits over workgroups.  Bit-identical to the sequential
 * recursion: out_nodes holds the reference's BVHNode array (root 0, node 1 padding,
 * children pairs in its order; capacity 2n + 2 nodes), out_order[i] the entry index at
 * position i of the partitioned entry array (BVHSortEntry::index).  Entries are the
 * centre p and half extent r of each primitive's or triangle's box (BVHSortEntry,
 * RT/bvh.h:25-29).  Host pointers; returns an rt_status (text: rt_build_bvh_last_error). */
enum rt_bvh_build_method {
    RT_BVH_BUILD_MIDPOINT   = 0,    /* BVH_MidpointSplit */
    RT_BVH_BUILD_SAH_BINNED = 1,    /* BVH_SAHBinned (16 bins) */
    RT_BVH_BUILD_SAH_FULL   = 2,    /* BVH_SAHFull: every entry's centre is a candidate split */
};
int rt_build_bvh(int device, uint32_t n, const rt_v3* p, const rt_v3* r, int method,
                 rt_bvh_node* out_nodes, uint32_t* out_node_count, uint32_t* out_order);
const char* rt_build_bvh_last_error(void);

/* Record per-stage HIP-event timings into rt_stats::kernel_ms (off by default). */
int rt_set_profiling(int enable);
/* The same for a subset of stages: bit k = stage k of rt_kernel_stage (other stages
 * record no events, so their launches are not slowed by the markers). */
int rt_set_profiling_stages(uint32_t mask);

/* Size of the in-flight path pool per partition (paths resident in HBM); 0 = default:
 * a fifth of the partition's samples, clamped to [2^21, 4 x 2^21]. */
int rt_set_path_pool(uint32_t paths);

/* How samples reach the accumulation buffer (splat_filter, RT/raytracer.cpp:187-259).
 *   RT_SPLAT_STREAM (default): each sample's 20-byte record goes to a ring of sample passes
 *     in HBM; k_resolve_tiles gathers completed passes into the buffer while the frame still
 *     renders, reading every record once.  Deterministic (the same bits whatever the timing
 *     or the split of passes between launches); equal to the reference's frame up to float
 *     summation order.
 *   RT_SPLAT_EXACT: records of the whole frame, then one gather in the reference's
 *     single-threaded order (tiles descending, pixels, samples): bit-identical to the
 *     reference order.  Over the HBM budget it renders as RT_SPLAT_STREAM.
 *   RT_SPLAT_ATOMIC: float atomics into the buffer (order-dependent last bits).
 * The mode a frame used is reported in rt_stats::splat_mode. */
enum rt_splat_mode {
    RT_SPLAT_STREAM = 0,
    RT_SPLAT_EXACT  = 1,
    RT_SPLAT_ATOMIC = 2,
};
int rt_set_splat_mode(int mode);

/* What rt_tile_set::shard_index / shard_count split a frame by (multi-GPU: one shard per rank,
 * the ranks' frames summed).  Either way every sample keeps its own key (frame, tile, pixel,
 * sample), so the shards' frames sum to the single-GPU frame up to float summation order.
 *   RT_SHARD_TILES (default): tile t belongs to shard t % shard_count (the reference's tile
 *     queue, RT/raytracer.cpp:551-560, dealt out round robin).
 *   RT_SHARD_PASSES: every tile, sample passes [spp*i/n, spp*(i+1)/n) of shard i of n: each
 *     shard sees the whole image, so the shards' costs match whatever the content.  The
 *     exact splat (RT_SPLAT_EXACT) is not split this way: such frames use RT_SPLAT_STREAM. */
enum rt_shard_mode {
    RT_SHARD_TILES  = 0,
    RT_SHARD_PASSES = 1,
};
int rt_set_shard_mode(int mode);

/* Environment-map importance sampling for next event estimation; 0 (default) = off.
 * The reference builds a luma CDF over 32 x 32 tiles of the environment map
 * (load_environment_map, RT/assets.cpp:620-665) but never samples it
 * (sample_environment_map is a stub, RT/integrators.cpp:230-233), so mode 0 is the
 * reference's estimator.  Mode 1, for scenes with an environment map and with
 * next_event_estimation on: a diffuse vertex's NEE picks the environment with probability
 * 1/2 (1 when the scene has no lights; a sphere light is then picked as before, its
 * probability halved), draws a tile with probability proportional to its luma (an alias
 * table built from the same tile sums at rt_scene_upload) and a uniform point in it, and
 * casts an unbounded shadow ray.  A path that leaves a diffuse vertex and escapes is
 * weighted against that pdf by the balance heuristic (use_mis; without MIS the
 * environment reaches diffuse vertices through the NEE only, as lights do in the
 * reference).  The estimate's expectation is unchanged; its noise is not the reference's.
 * No effect for scenes without an environment map (or one under 32 x 32 texels). */
int rt_set_env_sampling(int mode);

/* discard_current_render (RT/raytracer.cpp:686-690): polled between wavefront
 * iterations; the render in flight returns RT_ERROR_CANCELLED. */
int rt_cancel(rt_scene* scene);

/* Per-scene configuration of the wavefront schedule and the splat (none of it changes a
 * sample's bits; splat_mode and partitions change the float summation order of a pixel).
 * Two scenes in one process may differ.  rt_scene_upload starts a scene from
 * rt_scene_default_config(), then applies the test-override environment variables once
 * (RT_SPLAT, RT_PARTITIONS, RT_FUSE_PATHS, RT_SPLAT_CHUNK, RT_SPLAT_RING,
 * RT_SAMPLE_BUDGET_GB, RT_RES_TALL_PIXELS, RT_DEBUG_TRAVERSAL, RT_DRAIN_EVERY, RT_SHADOW_LAUNCH,
 * RT_RAMP_SHADE);
 * nothing reads the
 * environment per frame.  A field at RT_CONFIG_INHERIT follows the process-wide setter
 * above at each frame (rt_set_splat_mode / rt_set_shard_mode / rt_set_env_sampling /
 * rt_set_path_pool), so callers of those setters see no change. */
#define RT_CONFIG_INHERIT (-1)
/* rt_scene_config::shadow_launch (ABI 8): the shadow rays of an iteration's k_shade are traced in a launch
 * of their own right after it (SEPARATE), or in the next iteration's trace launch after its extension rays
 * (MERGED: one launch and one tail less per iteration; a finished path is splatted an iteration later).
 * AUTO: merged for a shard of a multi-rank frame (rt_tile_set::shard_count > 1), for path pools under
 * 4M paths (small frames), and for a whole frame on one GPU when the scene's previous frame traced at least
 * 0.15 shadow rays per extension ray (rt_stats::traced_rays); else separate -- a scene's first whole frame
 * is separate. */
typedef enum rt_shadow_launch {
    RT_SHADOW_LAUNCH_AUTO = 0,
    RT_SHADOW_LAUNCH_SEPARATE = 1,
    RT_SHADOW_LAUNCH_MERGED = 2
} rt_shadow_launch;
typedef struct rt_scene_config {
    int32_t  splat_mode;            /* rt_splat_mode, or RT_CONFIG_INHERIT                          */
    int32_t  shard_mode;            /* rt_shard_mode, or RT_CONFIG_INHERIT                          */
    int32_t  env_sampling;          /* 0 / 1, or RT_CONFIG_INHERIT                                  */
    int32_t  partitions;            /* concurrent partitions (streams) per frame, 1..8; 0 = auto (4) */
    int64_t  path_pool;             /* in-flight paths per partition; 0 = rt_set_path_pool / auto    */
    int64_t  fuse_paths;            /* fused drain below this many live paths; -1 = auto, 0 = never */
    int32_t  splat_chunk;           /* streaming splat: passes per resolve; 0 = auto                 */
    int32_t  splat_ring;            /* streaming splat: record-ring passes per partition; 0 = auto   */
    double   sample_budget_gb;      /* HBM for sample records; < 0 = auto (free HBM less 16 GB)      */
    int64_t  resolve_tall_pixels;   /* exact splat: 8-row gather strips from this many pixels; 0 = auto */
    int32_t  debug_traversal;       /* 1: each frame's TraversalStats and trace steps to stderr      */
    int32_t  traversal_ref;         /* 1: also count rt_stats::traversal_ref (the reference's units);
                                       the trace kernels then walk the top level in the reference's
                                       order (slower: no prologue mesh lists) -- a diagnostic mode  */
    int32_t  drain_every;           /* (ABI 8) fused-drain kernels ride on every Nth iteration once the
                                       host expects the drain (N >= 1; 0 = auto: every iteration).  A
                                       schedule knob for the tests: frames are identical for every N */
    int32_t  shadow_launch;         /* (ABI 8) rt_shadow_launch: where the NEE shadow rays are traced.
                                       Frames are identical for every value */
    int32_t  ramp_shade;            /* (one of ABI 8's reserved words) the dense shade launch of a frame's
                                       ramp-down, once every sample is claimed: 0 = auto (on), 1 = on,
                                       2 = off.  Frames are identical for every value */
    int32_t  reserved[3];
} rt_scene_config;
int rt_scene_default_config(rt_scene_config* out);
int rt_scene_get_config(const rt_scene* scene, rt_scene_config* out);
int rt_scene_set_config(rt_scene* scene, const rt_scene_config* config);

/* The traversal stack entries the scene's BVHs can need, as rt_scene_upload bounds them (read-only):
 * out_depth = top_depth + mesh_depth, where top_depth is the depth of the top-level BVH2 and mesh_depth the
 * largest bound over the meshes' BVH4s (a BVH4 node leaves up to 3 entries behind while its fourth child is
 * walked, so up to 3 per two BVH2 levels); out_depth_ref the same for a walk in the reference's units
 * (rt_scene_config::traversal_ref), which adds a marker per BVH4 level.  The stack holds 64 entries:
 * rt_scene_upload refuses a scene with out_depth + 2 > 64, and traversal_ref is refused when
 * out_depth_ref + 2 > 64.  This is the device's own bound: the reference's node_stack[64]
 * (RT/intersection.cpp:445) holds BVH2 entries, at most one per level, so it walks some BVH2s (from depth 43
 * on) that are refused here. */
int rt_scene_stack_depth(const rt_scene* scene, uint32_t* out_depth, uint32_t* out_depth_ref);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
