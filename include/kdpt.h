/*
 * kdpt.h -- C-ABI drop-in boundary of the MI355X (gfx950) KD-tree path tracer.
 *
 * Replaces the reference's device entry points (src/pathtrace.h:6-21):
 *   pathtraceInit(Scene*, bool enablekd)   -> kdpt_create
 *   pathtrace(uchar4* pbo, int frame, int iter, ...13 flags)
 *                                          -> kdpt_trace_iteration (+ kdpt_read_image,
 *                                             kdpt_write_pbo for the uchar4 preview)
 *   pathtraceFree(Scene*, bool enablekd)   -> kdpt_destroy
 * Plain POD in, host pointers in, no HIP/torch types.  Every entry point returns
 * an int status (KDPT_OK == 0) instead of exit(1) (src/pathtrace.cu:42-60);
 * kdpt_last_error() gives the message.  One context per device; a context is
 * not re-entrant (like the reference's file-static device globals,
 * src/pathtrace.cu:92-98).
 *
 * The structs keep the reference's byte layouts so the
 * arrays the reference's host code builds (Scene::newNodesBare,
 * Scene::newTrianglesBare, Scene::geoms, Scene::materials) pass through as is.
 */
#ifndef KDPT_H
#define KDPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDPT_OK 0
#define KDPT_ERR_ARG -1
#define KDPT_ERR_HIP -2
#define KDPT_ERR_UNSUPPORTED -3
#define KDPT_ERR_IO -4

/* struct Geom, src/sceneStructs.h:22-31 (236 bytes, glm::mat4 column-major) */
typedef struct kdpt_geom {
    int type; /* enum GeomType: 0 SPHERE, 1 CUBE */
    int materialid;
    float translation[3];
    float rotation[3];
    float scale[3];
    float transform[16];
    float inverseTransform[16];
    float invTranspose[16];
} kdpt_geom;

/* struct Material, src/sceneStructs.h:33-44 (56 bytes) */
typedef struct kdpt_material {
    float color[3];
    float specular_exponent;
    float specular_color[3];
    float hasReflective;
    float hasRefractive;
    float indexOfRefraction;
    float emittance;
    float transmittance[3];
} kdpt_material;

/* struct Camera, src/sceneStructs.h:46-55 (84 bytes) */
typedef struct kdpt_camera {
    int resolution[2];
    float position[3];
    float lookAt[3];
    float view[3];
    float up[3];
    float right[3];
    float fov[2];
    float pixelLength[2];
} kdpt_camera;

/* KDN::NodeBare, src/KDnode.h:64-82 (64 bytes) */
typedef struct kdpt_node_bare {
    int axis;
    float splitPos;
    float mins[3];
    float maxs[3];
    int ID;
    int parentID;
    int leftID;
    int rightID;
    int triIdStart;
    int triIdSize;
    float tmin;
    float tmax;
} kdpt_node_bare;

/* KDN::TriBare, src/KDnode.h:51-62 (76 bytes) */
typedef struct kdpt_tri_bare {
    float x1, x2, x3, y1, y2, y3, z1, z2, z3;
    float nx1, nx2, nx3, ny1, ny2, ny3, nz1, nz2, nz3;
    int mtlIdx;
} kdpt_tri_bare;

/* struct PathSegment (+ Ray), src/sceneStructs.h:15-20,65-71 (56 bytes) */
typedef struct kdpt_path_segment {
    float origin[3];
    float direction[3];
    uint8_t isinside;
    uint8_t pad_[3];
    float sdepth;
    float color[3];
    int pixelIndex;
    int remainingBounces;
    int materialIdHit;
} kdpt_path_segment;

/* struct ShadeableIntersection, src/sceneStructs.h:81-85 (20 bytes) */
typedef struct kdpt_shadeable_intersection {
    float t;
    float surfaceNormal[3];
    int materialId;
} kdpt_shadeable_intersection;

/* Everything pathtraceInit reads from Scene (src/pathtrace.cu:201-272). */
typedef struct kdpt_scene {
    kdpt_camera camera;        /* hst_scene->state.camera (after runCuda's camera update) */
    int traceDepth;            /* hst_scene->state.traceDepth */
    const kdpt_geom *geoms;
    int num_geoms;
    const kdpt_material *materials;
    int num_materials;
    int has_obj;               /* hst_scene->hasObj */
    const kdpt_node_bare *nodes; /* hst_scene->newNodesBare (ID order) */
    int num_nodes;
    const kdpt_tri_bare *tris; /* hst_scene->newTrianglesBare */
    int num_tris;
    const int *obj_materialOffsets; /* one per OBJ shape */
    int num_shapes;
    /* enable_kd = 0 only (brute force, pathTraceOneBounce src/pathtrace.cu:402-628): the raw OBJ arrays
       pathtraceInit uploads in that mode (src/pathtrace.cu:225-257), as Scene::loadObj builds them
       (src/scene.cpp:603-712).  Ignored when enable_kd = 1. */
    const float *obj_verts;      /* attrib.vertices: 3 floats per vertex index */
    int num_obj_verts;           /* floats */
    const float *obj_norms;      /* attrib.normals, read at 3*vertex_index like the reference */
    int num_obj_norms;           /* floats */
    const int *obj_polyoffsets;  /* per shape: number of vertex indices (3 per triangle) */
    const int *obj_polysidxflat; /* vertex indices, shape after shape */
    int polyidxcount;
    const float *obj_bboxes;     /* Scene::obj_bboxes; shape i's box is read at [i .. i+5] (use_bbox) */
    int num_bbox_floats;
} kdpt_scene;

/* The flags of pathtrace() with src/main.cpp:35-60 defaults (kdpt_default_options). */
typedef struct kdpt_options {
    float focal_length;  /* dofDistance, 6 */
    float dof_angle;     /* dofAngle, 0 */
    float softness;      /* 0 */
    int cacherays;       /* 0: regenerate camera rays every iteration */
    int antialias;       /* 1 */
    int enable_sss;      /* 0 */
    int testing_mode;    /* 0: 1 = also time the intersect kernel per bounce (TESTINGMODE) */
    int compaction;      /* 1 */
    int enable_kd;       /* 1; 0 = brute force over the OBJ arrays (pathTraceOneBounce) */
    int viz_kd;          /* 0; 1 = KD node boxes drawn as boxes (pathTraceOneBounceKDbareBoxes) */
    int use_bbox;        /* 0; brute force only: each shape's bbox test first (src/pathtrace.cu:497-513) */
    int short_stack;     /* 1: traverseKDbareShortHybrid, 0: traverseKDbare */
    int bounce_cap;      /* 8 == `depth > 7` (src/pathtrace.cu:2608); 16 for the stress config */
    int block_size;      /* 0 = default (256) */
    float *external_image; /* optional device float[3*W*H] to accumulate into (e.g. an RCCL buffer) */
} kdpt_options;

typedef struct kdpt_stats {
    long long segments;          /* sum over bounces of paths launched into the intersect kernel */
    long long seg_per_bounce[32];
    int bounces;                 /* bounces launched in the last iteration */
    int iterations;              /* iterations traced since create/reset */
    float ms_last_iteration;     /* hipEvent time of the last kdpt_trace_iteration (gen .. last gather) */
    float ms_intersect;          /* testing_mode: sum of intersect-kernel time, last iteration */
    long long total_segments;    /* since create/reset */
    double intersect_ms_total;   /* testing_mode: intersect-kernel time summed over launches since reset */
    long long intersect_launches_total; /* ... and the number of those launches */
    double intersect_device_ms_total;   /* intersect launches on the device clock (first block start to
                                           last block end), summed since reset -- unlike the events,
                                           not inflated by queueing when iterations overlap */
    long long intersect_device_launches_total;
    float intersect_grid_share;  /* fraction of the persistent intersect grid one launch used in the last
                                    kdpt_trace_iterations (1 for one-at-a-time tracing) */
    long long total_trace_rays;  /* since create/reset: rays handed to the KD traversal kernel (k_trace), i.e.
                                    the segments whose ray meets the KD root box */
    double create_ms;            /* host wall time of kdpt_create (uploads, cluster build, masks, kernel setup) */
    double mask_build_ms;        /* ... of which the masked cull's direction masks (built on the device; 0: none) */
} kdpt_stats;

typedef struct kdpt_ctx kdpt_ctx;

void kdpt_default_options(kdpt_options *opt);

/* pathtraceInit: allocate + upload (geoms, materials, nodes, triangles, offsets).
 * All argument and scene errors (KDPT_ERR_ARG / KDPT_ERR_UNSUPPORTED: options, resolution, KD tree shape,
 * triangle and OBJ arrays, geom types and materials) are reported before any device work, so they read the
 * same on a machine without a device; KDPT_ERR_HIP can only follow an accepted scene. */
int kdpt_create(const kdpt_scene *scene, const kdpt_options *opt, int device, kdpt_ctx **out);
/* pathtrace(pbo, frame, iter, ...): one iteration (1 sample per pixel); iter is 1-based and
 * seeds the RNG.  Synchronous on return, like the reference.
 * KDPT_ERR_UNSUPPORTED (from every entry point that shades, before anything is queued) for a KD-traversed OBJ
 * with triangles of a shape other than the first: the reference's traversal reports material
 * mtlIdx + material_size - 1 for their hits (src/pathtrace.cu:1142), past the end of its materials array, so
 * there is no defined result to reproduce.  kdpt_cast_rays (which only reports that number) and enable_kd = 0
 * (which takes the material from the shapes' offsets) remain available. */
int kdpt_trace_iteration(kdpt_ctx *ctx, int frame, int iter);
/* Iterations first_iter + k*stride (k < count), in batches of `batch` (<= 16) that share each bounce's
 * intersect launch, with `pipeline` batches in flight at once (each on its own stream and buffers).
 * Partial images are added into the image in iteration order, so the result is bit-identical to
 * calling kdpt_trace_iteration for each.  Returns after enqueueing; follow with kdpt_synchronize.
 * Stats: iterations, total_segments and the intersect totals. */
int kdpt_trace_iterations(kdpt_ctx *ctx, int frame, int first_iter, int count, int stride, int pipeline,
                          int batch);
/* As kdpt_trace_iteration but returns after enqueueing (no host sync, no stats). */
int kdpt_trace_iteration_async(kdpt_ctx *ctx, int frame, int iter);
int kdpt_synchronize(kdpt_ctx *ctx);
/* The float3 accumulation image (sum over iterations, not averaged): 3*W*H floats. */
int kdpt_read_image(kdpt_ctx *ctx, float *rgb);
/* sendImageToPBO (src/pathtrace.cu:69-89) into uchar4[W*H] (x,y,z,w bytes).  `rgba` may be device memory
 * (the reference's GL-mapped PBO: written by the kernel directly) or host memory (copied out through a
 * staging buffer the context keeps).  Synchronous. */
int kdpt_write_pbo(kdpt_ctx *ctx, int iter, uint8_t *rgba);
int kdpt_reset(kdpt_ctx *ctx);

/* ---- Headless output (saveImage, src/main.cpp:1087-1108 + image::savePNG/saveHDR, src/image.cpp:22-45) ---- */
/* The bytes savePNG encodes: x-flipped, image / samples, glm::clamp(0, 1) * 255.f, (unsigned char). */
int kdpt_save_rgb8(kdpt_ctx *ctx, float samples, uint8_t *rgb);
/* image::savePNG / image::saveHDR of the current image (stb_image_write's encoders, restated). */
int kdpt_save_png(kdpt_ctx *ctx, const char *path, float samples);
int kdpt_save_hdr(kdpt_ctx *ctx, const char *path, float samples);
/* The encoders alone (host; no device needed).  *out is malloc'd: release with kdpt_free. */
int kdpt_png_encode(const uint8_t *rgb, int w, int h, uint8_t **out, size_t *len);
int kdpt_write_png(const char *path, const uint8_t *rgb, int w, int h);
int kdpt_hdr_encode(const float *rgb, int w, int h, uint8_t **out, size_t *len);
int kdpt_write_hdr(const char *path, const float *rgb, int w, int h);
void kdpt_free(void *p);
int kdpt_get_stats(kdpt_ctx *ctx, kdpt_stats *st);
/* pathtrace()'s per-call flags without a new context: focal_length, dof_angle, softness, cacherays,
 * antialias, enable_sss, testing_mode, compaction and short_stack take effect from the next iteration
 * (the accumulation image is kept).  enable_kd, viz_kd, use_bbox, bounce_cap, block_size and
 * external_image must equal the context's (KDPT_ERR_UNSUPPORTED otherwise: they decide what
 * kdpt_create uploads and allocates). */
int kdpt_set_options(kdpt_ctx *ctx, const kdpt_options *opt);
/* Explicit A/B and diagnostic knobs (the library reads no environment variables; a context created
 * without this call always runs the tested default route).  Names: "shade_fused" (1; 0 = k_shade +
 * k_scan + k_scatter), "early_walk" (16) / "early_leaf" (1) (node-phase hand-over thresholds),
 * "chunk_width0..2" (16, 64, 64), "trace_grid_frac" (grid share of every intersect launch, (0, 1]),
 * "tree_global" (0; 1 = KD tree read from HBM/L2 instead of LDS), "profile_batches" (0; 1 = counting intersect kernel for kdpt_wave_profile, 2 = also its
 * per-ray node-step histogram),
 * "shade_batch" (1; 0 = one k_shade_fused launch per iteration instead of one per batch), "gen_geoms" (1;
 * 0 = camera rays and bounce 0's k_geoms as two launches instead of one k_gen_geoms_b),
 * "tree_format" (0 = best fit; 16 / 32 = only that LDS record size), "super_cull" (1; 0 = no two-level
 * super-cluster route), "cluster_slab" (1; 0 = no normal slab in the second cull level), "cluster_obb" (1;
 * 0 = the second level tests the axis-aligned box and the normal slab only, not the oriented box),
 * "super_slab" (1; 0 = the first level tests the super-clusters' boxes only, not their slabs),
 * "flat_obb" (1; 0 = the one-level cluster cull tests the clusters' axis-aligned boxes only, not also
 * their oriented boxes),
 * "cluster_cull" (1; 0 = no cluster / chunk cull at all: every big-leaf cluster is swept, exact by
 * construction), "cull_margin" (0 = the scene's; > 0 overrides the cull's margin coefficient, no masks),
 * "cull_exact" (1; 0 = for meshes of large triangles the margin-only cull instead of the masked exact one, not
 * exact), "cull_mask_n" (the direction masks' cube-map cells per face edge, 1 .. 512; default: the finest of
 * 256 / 128 / 64 ... within 640 MB; KDPT_ERR_ARG, and the current masks kept, when 6 n^2 num_clusters >= 2^32: the
 * kernel indexes the table with 32 bits), "cull_fast_k" (the masked cull's box coefficient, default 1e-3; the masks
 * are rebuilt for it), "reduce_spin_us" (0; > 0: a device spin of that many
 * microseconds on the reduce stream before every frame's reduce, emulating an ncclReduce that waits for a slower
 * peer -- a diagnostic of the frame pipeline; ctx = NULL sets it for contexts created later, e.g. the ones
 * kdpt_render_sharded creates), "sync_debug" (0), "cast_chunk" (1 << 20; the rays per chunk of kdpt_cast_rays, at
 * least 64: its buffers are remade on the next call).  ctx = NULL only (process defaults of the contexts created afterwards):
 * "cluster_chord" (-1: normal cones of chord 0.02 before the Morton runs for meshes whose cull margin is
 * rigorous, Morton runs only otherwise; 0: Morton runs only; > 0: cones of that chord for every mesh -- the
 * cluster layout, same bits), "cu_mask_streams" (1: the context's streams are created with a mask of every CU,
 * each on a hardware queue of its own; 0: plain non-blocking streams, which HIP multiplexes onto
 * GPU_MAX_HW_QUEUES in-order queues).  KDPT_ERR_ARG for an unknown name.  Drops the pipeline slots
 * (they are remade). */
int kdpt_set_tuning(kdpt_ctx *ctx, const char *name, double value);
/* The intersect kernel's configuration: tree source (0 HBM 64-byte records, 1 HBM 32-byte, 2 LDS 32-byte,
 * 3 LDS 16-byte derived-box records + cluster boxes, 4 LDS 16-byte records with cluster boxes in HBM,
 * 5 LDS 16-byte records + super-cluster records (half-precision boxes rounded outward; cluster boxes and
 * normal slabs in HBM, culled in two levels)), workgroup size, persistent grid (workgroups of the full grid)
 * and dynamic LDS bytes per workgroup. */
int kdpt_trace_config(kdpt_ctx *ctx, int *tree_mode, int *block, int *grid, long long *lds_bytes);
/* The big-leaf cluster cull (and the brute-force chunk cull): the margin coefficient in use, the scene's
 * rigorous coefficient, and exact = 1 when the one in use is >= the rigorous one -- the cull then never
 * drops a cluster holding a triangle that passes glm's u/v tests, for any ray ("Cluster cull").
 * For meshes whose triangles are too large for a rigorous margin that still culls (dragon_5), the box levels
 * use a fast coefficient and per-cluster direction masks decide the missed pairs' near-parallel triangles
 * one by one (the masked cull): exact = 1 as well.  exact = 0 after tuning "cull_exact" = 0 or a fixed
 * "cull_margin": the cull is then conservative except for rays nearly coplanar with a triangle.  The brute-force
 * route (enable_kd = 0) has no masks: each of its 64-triangle chunks is culled at the rigorous coefficient of its
 * own triangles (never, when that could cull nothing), so exact = 1 and margin is the smallest of those
 * coefficients (+inf when no chunk is culled), unless a knob fixes one. */
int kdpt_cull_margin(kdpt_ctx *ctx, float *margin, double *rigorous, int *exact);
/* Report only: *staged = 1 when the fused shading kernels run with the scene's analytic geoms and materials copied
 * to LDS (at most 8 geoms, KD boxes of viz_kd included, and at most 32 materials), 0 when they read them from
 * memory. */
int kdpt_shade_staged(kdpt_ctx *ctx, int *staged);
/* The masked cull's danger masks as the device built them (bucket-major: cell b * num_clusters + c, 6 mask_n^2
 * buckets).  *mask_n = 0 when the scene has none (its cull is exact without them).  masks may be NULL (sizes
 * only); otherwise 6 mask_n^2 num_clusters entries.  For parity tests against the host builder
 * (kdpt_clusters.h build_dir_masks). */
int kdpt_cull_masks(kdpt_ctx *ctx, int *mask_n, int *num_clusters, unsigned long long *masks);

/* ---- Multi-GPU: samples per pixel sharded across GPUs ----
 * Frame f covers global iterations f*spp + 1 .. (f+1)*spp (the RNG seeds, iteration 2's sort and cacherays
 * use these numbers); rank r of N renders those with (iteration - 1 - f*spp) % N == r, in order, into a frame
 * buffer, and one reduce (float sum, to rank 0) per frame over xGMI combines them.  Rank 0 adds each frame
 * into its context's image (kdpt_read_image, kdpt_save_png) and copies it to `out` when given.  With one
 * rank, one frame and a zero image, the image equals kdpt_trace_iterations(first, spp, stride 1) bit for bit;
 * with N ranks it equals the rank partial sums added in the reduce's order.  The calls queue their work and
 * return (kdpt_synchronize waits); frame f + 1 renders while frame f is reduced.  RCCL (librccl.so.1) is
 * loaded at run time; KDPT_ERR_UNSUPPORTED when it is absent.
 * Replaces the reference's single-GPU pathtrace() loop (src/pathtrace.cu:2405-2635, src/main.cpp runCuda). */
#define KDPT_COMM_ID_BYTES 128
#define KDPT_REDUCE_RCCL 0  /* ncclReduce (one communicator rank per context) */
#define KDPT_REDUCE_COPY 1  /* in-process: peer copies to the first device, added in rank order */
/* One process per GPU: rank 0 makes the id, the caller hands it to every rank (any channel), and each rank
 * joins with its context (collective: every rank must call it).  An id is single-use: every communicator (every
 * kdpt_comm_init round over the ranks) needs a fresh kdpt_comm_unique_id -- reusing one makes RCCL fail
 * ("remote process exited or there was a network error").  id = NULL with nranks > 1: no
 * communicator; kdpt_render_frames then copies every rank's frame shares to its `out` and the caller reduces
 * them (e.g. over gloo when ranks share a GPU, which RCCL refuses); the image is left alone. */
int kdpt_comm_unique_id(unsigned char *id);
/* id given: a communicator for any nranks >= 1 (one rank runs the same per-frame ncclReduce as N). */
int kdpt_comm_init(kdpt_ctx *ctx, int nranks, int rank, const unsigned char *id);
/* The path of the RCCL library whose ncclReduce the calls use (dladdr; in a torch process torch's copy when
 * it was loaded first).  KDPT_ERR_UNSUPPORTED when no librccl.so.1 can be loaded. */
int kdpt_comm_library(char *path, int len);
/* This rank's share of frames first_frame .. first_frame + frames - 1 (every rank calls it with the same
 * arguments); out: rank 0, frames * 3*W*H floats, device or host memory, or NULL. */
int kdpt_render_frames(kdpt_ctx *ctx, int first_frame, int frames, int spp, int pipeline, int batch, float *out);
/* (a pageable host `out` is pinned for the copies -- hipHostRegister -- until kdpt_synchronize; it must stay
 * allocated until kdpt_synchronize returns, and two contexts must not render into one `out` range at once) */
/* One process, one context per device (devices[0..ndev), <= 8; a device may repeat with KDPT_REDUCE_COPY):
 * renders the frames, waits, and frees everything.  out (host or device 0 memory, frames * 3*W*H floats, or
 * NULL) receives each frame's reduced image. */
int kdpt_render_sharded(const kdpt_scene *scene, const kdpt_options *opt, int ndev, const int *devices,
                        int first_frame, int frames, int spp, int pipeline, int batch, int reduce, float *out);

/* ---- Ray queries: closest hits for caller-supplied rays ----
 * Record i is what pathTraceOneBounceKDbare (src/pathtrace.cu:1489-1662) computes for ray i before scatterRay:
 * the analytic geoms, then the KD traversal the context's short_stack option selects (traverseKDbareShortHybrid
 * or traverseKDbare), on the context's current tree route, cull and tuning knobs -- the hit the path tracer
 * gets for the same ray, bit for bit.  Closest hit only, with the reference's semantics (its single-sided
 * triangle test, the hybrid walk's skip line).  There is no t_max and no any-hit mode: the hybrid walk's
 * visiting order depends on the hits found so far, so a bounded query would not equal "this hit, filtered".
 *
 * origins / directions: 3*n floats each; out: n records; each pointer may be host memory or memory of the
 * context's device (told apart with hipPointerGetAttributes, as kdpt_write_pbo does).  n == 0 returns KDPT_OK
 * and touches nothing; n < 0, a null pointer with n > 0 or an unknown flag bit is KDPT_ERR_ARG.
 *
 * Directions must be unit length: the cluster cull takes n . d as a cosine ("Cluster cull"), so
 * this is a correctness condition.  With KDPT_CAST_NORMALIZE each direction first goes through the
 * reference's glm::normalize (t is then along the unit direction).  Without it a direction is accepted only
 * when |dot(d, d) - 1| <= 1e-6 in float arithmetic: every output of the float normalize passes (its three
 * roundings keep the squared length within about 6e-7 of 1), nothing much longer or shorter than what the
 * path tracer itself traces does, and the cull's margins hold for that range ("Ray queries").
 * A ray with a non-finite origin or direction component, a zero direction, a direction whose normalisation is
 * not finite or (without the flag) a non-unit direction is rejected: its record has kind KDPT_HIT_INVALID and
 * it is never traced, whether the arrays live on the host or on the device.
 *
 * Synchronous: waits for the work already queued on the context (as kdpt_synchronize does), runs, and
 * returns with `out` filled.  The accumulation image, kdpt_stats, the iteration counter, the pipeline slots
 * and every buffer of the render path are left alone.  The rays go through in chunks of "cast_chunk" rays
 * (kdpt_set_tuning; default 1 << 20, at least 64) whatever the image resolution; the query's buffers are
 * allocated on first use.  KDPT_ERR_UNSUPPORTED for contexts with enable_kd = 0 or viz_kd = 1. */
#define KDPT_HIT_INVALID  -1   /* the ray was rejected (see above); never traced */
#define KDPT_HIT_NONE      0
#define KDPT_HIT_GEOM      1   /* prim = index into scene->geoms */
#define KDPT_HIT_TRIANGLE  2   /* prim = index into scene->tris (TriBare order) */
typedef struct kdpt_ray_hit {  /* 40 bytes */
    float t;          /* the reference's t_min of the winning hit; -1 when kind <= 0 */
    int kind;
    int prim;         /* -1 when kind <= 0 */
    int material;     /* geoms[prim].materialid, or the triangle's objMaterialIdx; -1 when kind <= 0 */
    float point[3];   /* intersect_point, as pathTraceOneBounceKDbare hands it to scatterRay; 0 when kind <= 0 */
    float normal[3];  /* likewise the normal */
} kdpt_ray_hit;

#define KDPT_CAST_NORMALIZE 1  /* apply the reference's glm::normalize to each direction first */
int kdpt_cast_rays(kdpt_ctx *ctx, const float *origins, const float *directions, long long n,
                   int flags, kdpt_ray_hit *out);
/* Since create/reset: the rays cast, those of them that reached the KD traversal kernel (their ray meets the
 * KD root box; rejected rays never do), and the last kdpt_cast_rays' time on the device (hipEvents around its
 * launches and staging copies on the context's stream). */
int kdpt_cast_stats(kdpt_ctx *ctx, long long *rays, long long *traced, double *device_ms);

/* ---- Caller-defined views: set the camera, read its rays, or path trace rays of your own ----
 * kdpt_set_camera replaces the pinhole camera the context was created with, from the next enqueued iteration
 * on (launches take the camera by value, so iterations already queued keep theirs; no device work, no
 * synchronisation).  The accumulation image, kdpt_stats and the iteration counter are kept, as kdpt_set_options
 * keeps them: kdpt_reset clears them.  camera->resolution must equal the context's (everything sized by W*H
 * stays) and every float must be finite; anything else is KDPT_ERR_ARG and the old camera stays.
 *
 * kdpt_camera_rays returns the W*H rays generateRayFromCamera (src/pathtrace.cu:315-397) produces for iteration
 * `iter` (>= 1) with the context's current camera and options (antialias, dof_angle, focal_length; with
 * cacherays, iteration 1's rays whatever `iter`), as the device computes them: 3*W*H floats each, ray
 * y*W + x at [3 (y*W + x)].  Each output may be host memory or memory of the context's device.  Synchronous;
 * the render state is left alone.
 *
 * kdpt_trace_rays path traces n caller-supplied rays.  For each iteration first_iter + k (k < count) it runs
 * what kdpt_trace_iteration runs with the camera stage replaced: path i starts as {origins[i], directions[i],
 * colour (1, 1, 1), pixelIndex i, remainingBounces traceDepth}, there are n paths instead of W*H, and everything
 * after that is the context's own pipeline -- its options (compaction, iteration 2's sort, softness, SSS,
 * short_stack, bounce_cap), its tree route, cull and knobs, and the RNG seeds (iteration, slot, depth) as they
 * fall.  The result is the reference's render of an n-pixel image whose camera had produced these rays: fed
 * kdpt_camera_rays' output, it reproduces kdpt_trace_iteration's image bit for bit.  radiance (3*n floats, host
 * or device memory) is overwritten with the sum over the iterations, in iteration order, of what the gathers add
 * to pixel i.
 *
 * n <= W*H of the context, else KDPT_ERR_ARG: the path buffers hold W*H paths, and the shading seeds its RNG
 * with a path's compacted slot, so tracing more rays in chunks would not give the result of tracing them
 * together.  A caller who needs more rays per call creates a context of a larger resolution.  n == 0 or
 * count == 0 returns KDPT_OK and touches nothing; n < 0, count < 0, first_iter < 1, a null pointer with work to
 * do or an unknown flag bit is KDPT_ERR_ARG, reported before any device call.
 *
 * flags: KDPT_CAST_NORMALIZE, with kdpt_cast_rays' meaning, and without it the same acceptance rule
 * (|dot(d, d) - 1| <= 1e-6 in float, finite components; kdpt_camera_rays' directions pass it).  A rejected ray
 * is never traced: its path is born finished with a NaN colour, which the gather adds, so its radiance is NaN in
 * all three channels (the analogue of KDPT_HIT_INVALID); the other rays' results do not depend on it when
 * compaction is off, and with compaction on only through the slots the survivors are compacted into.
 *
 * Supported wherever kdpt_trace_iteration is (KD hybrid and bare walks, enable_kd = 0, viz_kd = 1), with the
 * same KDPT_ERR_UNSUPPORTED refusal.  Synchronous, as kdpt_cast_rays is: waits for the work queued on the
 * context, runs on the context's stream, and returns with radiance filled.  The accumulation image, kdpt_stats
 * (total_segments, total_trace_rays and the intersect totals included), the iteration counter, the pipeline
 * slots and kdpt_cast_rays' buffers are left alone: the query has an iteration state of its own, allocated on
 * first use.  As in a render with compaction = 0, iteration 2's sort orders finished paths by the material id
 * their slot last held, which for a query is what the query state's previous use left there. */
int kdpt_set_camera(kdpt_ctx *ctx, const kdpt_camera *camera);
int kdpt_camera_rays(kdpt_ctx *ctx, int iter, float *origins, float *directions);
int kdpt_trace_rays(kdpt_ctx *ctx, const float *origins, const float *directions, long long n,
                    int first_iter, int count, int flags, float *radiance);
/* Of the last kdpt_trace_rays on the context (the query's own totals; kdpt_stats never sees them): the path
 * segments launched into the intersect stage summed over its iterations (kdpt_stats.total_segments' meaning),
 * those of them handed to the KD traversal kernel (total_trace_rays' meaning), and the call's time on the device
 * (hipEvents on the context's stream, from the zeroing of the radiance buffer to the copy out of it). */
int kdpt_trace_rays_stats(kdpt_ctx *ctx, long long *segments, long long *traced, double *device_ms);

/* ---- Second moments: per-pixel variance, a noise map and a stopping estimate ----
 * A render accumulates S = sum of c over the iterations (the image).  With moments on the context also keeps
 * Q = sum of c^2 (sumsq, 3*W*H floats, the image's layout) and the number of iterations added since both were
 * zeroed.  For every iteration added to the image and each of its 3*W*H floats, with x that iteration's partial
 * value: the image gets x exactly as with moments off (same bits), and sumsq = fadd(sumsq, fmul(x, x)), two
 * float32 roundings, never a fused multiply-add, denormals kept, in the same iteration order as the image's adds.
 * The oracle renders single iterations, so sumsq is checkable as a bit pattern.
 *
 * kdpt_set_moments(ctx, 1) allocates sumsq (zero) and the counter (0).  It is accepted only while nothing has
 * been added to the image since kdpt_create / kdpt_reset (kdpt_stats.iterations == 0, and no
 * kdpt_trace_iteration_async or frame either); otherwise KDPT_ERR_UNSUPPORTED -- call kdpt_reset first -- and
 * nothing changes: the image and the moments must describe the same samples.  enable = 0 waits for the queued work
 * and frees the buffers; the context is then what it was before.  Setting the state it already has is KDPT_OK.
 * kdpt_reset zeroes sumsq and the counter with the image; kdpt_set_options, kdpt_set_camera and kdpt_set_tuning
 * keep them, as they keep the image; kdpt_destroy frees them.
 *
 * While moments are on: kdpt_trace_iterations adds each batch with a kernel that reads and writes the image and
 * sumsq once per batch; kdpt_trace_iteration[_async] gathers into a partial image of the context's, added the
 * same way (image bits, kdpt_stats and ms_last_iteration keep their meaning); kdpt_render_frames on the context
 * returns KDPT_ERR_UNSUPPORTED before anything is queued (frames reach the image through a cross-rank reduce that
 * does not carry second moments; kdpt_render_sharded makes contexts of its own and is unaffected).
 * kdpt_count_iteration, kdpt_debug_paths, kdpt_cast_rays, kdpt_trace_rays[_moments] and kdpt_camera_rays touch
 * neither the image nor the moments.  With moments off every path is the one it was.
 *
 * kdpt_read_moments copies sumsq (3*W*H floats, host memory; may be NULL) and reports the counter (may be NULL),
 * after the pipelined adds queued so far.  KDPT_ERR_UNSUPPORTED while moments are off.
 *
 * kdpt_noise_map writes, for each pixel p, the relative standard error of its mean, computed on the device in
 * double arithmetic from the float sums in exactly this order (S = image, Q = sumsq, c = r, g, b):
 *   n = (double)samples;  m_c = (double)S_c / n;  v_c = ((double)Q_c - (double)S_c * m_c) / (n - 1), < 0 -> 0;
 *   mbar = ((m_r + m_g) + m_b) / 3;  vbar = ((v_r + v_g) + v_b) / 3;  d = mbar > floor ? mbar : floor;
 *   noise[p] = (float)(sqrt(vbar / n) / d)
 * (W*H floats, host memory or memory of the context's device, told apart as kdpt_write_pbo does).  A NaN sum
 * gives a NaN entry; a pixel that only ever saw black gives exactly 0.  `floor` keeps dark pixels from dominating
 * and must be finite and > 0, and at least 2 iterations must have been accumulated: KDPT_ERR_ARG otherwise;
 * KDPT_ERR_UNSUPPORTED while moments are off.  Synchronous; the render state is left alone.  The float32 sums carry
 * their own rounding (about 2^-24 sqrt(n) relative each), so Q - S^2/n is meaningful only down to a relative
 * variance of about 1e-6 sqrt(n): below that the estimate is rounding noise (clamped at 0), not signal.
 *
 * kdpt_noise_estimate reduces the same per-pixel values on the device: pixels = W*H, nonfinite = the entries that
 * are NaN or inf, max and mean over the finite entries (the mean summed in double; 0 when there is none), above =
 * the finite entries > threshold (NaN: KDPT_ERR_ARG).  Other errors as kdpt_noise_map.  The reduction has a fixed
 * order and uses no floating-point atomics: two calls on the same state return identical bytes, so a stopping rule
 * built on it is reproducible. */
int kdpt_set_moments(kdpt_ctx *ctx, int enable);
int kdpt_read_moments(kdpt_ctx *ctx, float *sumsq, long long *samples);
int kdpt_noise_map(kdpt_ctx *ctx, float floor, float *noise);
typedef struct kdpt_noise {  /* 48 bytes */
    long long samples, pixels, above, nonfinite;
    double mean;   /* over the finite pixels */
    float max;     /* over the finite pixels */
    float pad_;
} kdpt_noise;
int kdpt_noise_estimate(kdpt_ctx *ctx, float floor, float threshold, kdpt_noise *out);
/* kdpt_trace_rays with one more output, and its contract for n, first_iter, count and flags, its acceptance rule,
 * the n <= W*H limit and what it leaves alone.  radiance is bit-equal to kdpt_trace_rays' for the same arguments;
 * sumsq[3 i + c] (3*n floats, host or device memory) is the sum over the call's iterations, in order, of
 * fl(x * x), x being what that iteration's gathers add to ray i -- so per-ray error bars take one call, not
 * `count` calls.  A rejected ray is NaN in both.  sumsq == NULL with work to do is KDPT_ERR_ARG.  Each iteration
 * gathers into a buffer of the query's own: nothing is shared with the render's moments, and the call works
 * whether kdpt_set_moments is on or off.  kdpt_trace_rays_stats reports it as it reports kdpt_trace_rays. */
int kdpt_trace_rays_moments(kdpt_ctx *ctx, const float *origins, const float *directions, long long n,
                            int first_iter, int count, int flags, float *radiance, float *sumsq);

/* ---- Adaptive sampling: re-trace only the pixels whose noise is above a threshold ----
 * State: a context with moments on gains extra[p], a uint32 per pixel, allocated (zero) by the first kdpt_active_pixels
 * or kdpt_trace_adaptive.  kdpt_reset zeroes it with the image and sumsq; kdpt_set_moments(ctx, 0) frees it;
 * kdpt_set_options, kdpt_set_camera and kdpt_set_tuning keep it.  Pixel p's sample count is n_p = samples + extra[p],
 * `samples` being kdpt_read_moments' counter of uniform iterations.  While extra is absent every other call does what
 * it did before; once it exists kdpt_noise_map and kdpt_noise_estimate use n_p in place of n (kdpt_noise.samples
 * stays the uniform count).
 *
 * Active rule: e_p is kdpt_noise_map's formula with n replaced by n_p, computed by the same device function in the
 * same operation order; pixel p is active iff isfinite(e_p) && e_p > threshold -- the rule behind kdpt_noise_estimate's
 * `above`, so a pixel whose sums are NaN or inf is never re-traced.  The active list A holds the active pixel indices
 * (y*W + x) in ascending order; it is built on the device by a flag pass and an ordered compaction without atomics,
 * so two calls on the same state give the same list.
 *
 * kdpt_active_pixels returns the list: *n = |A|, and pixels (|A| <= W*H ints; host memory or memory of the context's
 * device; may be NULL for the count alone) its entries.  Synchronous; the render state is left alone.
 *
 * kdpt_trace_adaptive is synchronous, as kdpt_trace_rays is: it waits for the work queued on the context (the
 * pipelined adds included), builds A once from the state before the call, reads |A| back (4 bytes: its only host read
 * before the end) and runs iterations first_iter + k (k < count) over A on kdpt_trace_iterations' batched, pipelined
 * route (pipeline and batch clamped as there; the result's bits do not depend on them).  With |A| = 0 or count = 0 it
 * returns KDPT_OK with out->pixels and out->active filled, and nothing changes.  For each iteration `it`, in order:
 * path j starts as the ray kdpt_camera_rays(it) returns for pixel A[j] (jitter, depth of field and the cacherays rule
 * included) with colour (1, 1, 1), pixelIndex j and remainingBounces traceDepth; there are |A| paths; everything
 * after that is the context's own pipeline with the RNG seeds (it, slot, depth) as they fall.  With x what that
 * iteration's gathers add to slot j, for each channel image[A[j]] = fadd(image[A[j]], x) and sumsq[A[j]] =
 * fadd(sumsq[A[j]], fmul(x, x)), and extra[A[j]] += 1.  That is, bit for bit, the composition
 *   o, d = kdpt_camera_rays(it) restricted to A;  r = kdpt_trace_rays_moments(o, d, |A|, it, 1, 0);  x_j = r_j
 * scattered through A; with A = every pixel, the image and sumsq of kdpt_trace_iterations(first_iter, count).
 * Supported wherever kdpt_trace_rays is, with the same KDPT_ERR_UNSUPPORTED refusal, and its caveat about iteration
 * 2's sort under compaction = 0 applies as written there.  kdpt_stats is left alone (iterations, total_segments and
 * the intersect totals do not move: the call's totals go to `out`, as a query's do), and so are the moments' `samples`
 * counter, kdpt_cast_rays' buffers and kdpt_trace_rays' state.  A later kdpt_set_moments(ctx, 1) asks for a reset, as
 * after any iteration.
 * Errors, reported before any device work: KDPT_ERR_ARG for first_iter < 1, count < 0, a null `out` or ctx, a floor
 * that is not finite and > 0, a NaN threshold or fewer than 2 uniform iterations accumulated; KDPT_ERR_UNSUPPORTED
 * while moments are off or the context is in a communicator (kdpt_comm_init: frames carry no per-pixel counts).
 * kdpt_active_pixels takes the same checks.
 * Pixels whose e_p reads exactly 0 after few samples (a pixel that saw the same value every time) are never
 * revisited: enough uniform iterations before the first adaptive call are the caller's guard.
 *
 * kdpt_read_sample_counts writes n_p (W*H ints, host memory); before any adaptive call every entry is `samples`.
 * kdpt_save_counted is kdpt_save_rgb8's pixel pass (rgb: 3*W*H bytes) and the floats kdpt_save_hdr writes (lin: 3*W*H
 * floats), either of which may be NULL, with each source pixel divided by (float)n_p instead of one `samples`: with
 * no extra samples bit-equal to kdpt_save_rgb8(ctx, (float)samples); a pixel with n_p = 0 gives 0.  Both return
 * KDPT_ERR_UNSUPPORTED while moments are off.
 * kdpt_selftest_active_list runs the list kernels' flag-and-compact part on npix caller-supplied values on device 0:
 * pixels (npix ints) receives the indices i with isfinite(noise[i]) && noise[i] > threshold, ascending, *n their
 * number. */
typedef struct kdpt_adaptive {   /* 48 bytes */
    long long pixels;            /* W*H */
    long long active;            /* |A| of this call */
    long long pixel_samples;     /* active * count */
    long long segments, traced;  /* kdpt_trace_rays_stats' meanings, summed over the call */
    double device_ms;            /* hipEvents on the context's stream, from after the list to after the last add */
} kdpt_adaptive;
int kdpt_active_pixels(kdpt_ctx *ctx, float floor, float threshold, int *pixels, long long *n);
int kdpt_trace_adaptive(kdpt_ctx *ctx, int first_iter, int count, int pipeline, int batch, float floor,
                        float threshold, kdpt_adaptive *out);
int kdpt_read_sample_counts(kdpt_ctx *ctx, int *counts);
int kdpt_save_counted(kdpt_ctx *ctx, uint8_t *rgb, float *lin);
int kdpt_selftest_active_list(const float *noise, int npix, float threshold, int *pixels, int *n);

/* ---- Denoising: a variance-guided edge-avoiding a-trous filter ----
 * The other use of the per-pixel variance: a cleaner image from the samples already spent.  The filter is the
 * spatial core of SVGF (Schied et al. 2017: the variance of each pixel steers its luminance tolerance, and is
 * filtered along) on the a-trous wavelet of Dammertz et al. 2010, without the temporal part.  Like the other
 * contracts here it is a bit pattern: float32 add, subtract, multiply, divide, sqrt, compare and abs only, every
 * operation rounded on its own (no fused multiply-add), denormals kept, no transcendental -- which is why the
 * edge-stopping function is the rational g below and not exp -- so a numpy float32 restatement gives the same bits.
 *
 * Inputs for a W x H image, pixel p = y*W + x: color[p][3], variance[p] (the variance of the pixel's mean),
 * normal[p][3], point[p][3], depth[p], id[p].  Pixel p is valid iff its 11 floats are finite, depth[p] > 0 and
 * variance[p] >= 0; validity is decided once, from the inputs, and holds for every pass.  An invalid pixel is never
 * a tap, and its own colour and variance pass through every pass unchanged, bit for bit.
 *
 * kdpt_denoise_params (kdpt_default_denoise_params fills the defaults): passes 0 .. 8 (5); normal_power_log2
 * 0 .. 10 (7: cos^128); sigma_l > 0 (4), sigma_z > 0 (0.02), eps_l > 0 (1e-8), all finite.  passes = 0 copies the
 * inputs to the outputs.
 *
 * Pass k = 0 .. passes-1, step s = 1 << k, reads pass k-1's colour and variance (the inputs for k = 0) and, for
 * every valid pixel p = (x, y):
 *   prefilter: g3 = [1/4, 1/2, 1/4]; for dy = -1..1 (outer), dx = -1..1 (inner), always at step 1, over the taps q
 *     inside the image and valid: sg = sg + g3[dy+1] g3[dx+1];  sv = sv + (g3[dy+1] g3[dx+1]) variance[q];
 *     sd = sqrt(sv / sg)
 *   lum(c) = ((c.r + c.g) + c.b) / 3;  den_l = sigma_l sd + eps_l;  den_z = sigma_z depth[p];
 *   g(x) = 1 / (1 + x (1 + 0.5 x))
 *   taps: h = [1/16, 1/4, 3/8, 1/4, 1/16]; for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + s dx, y + s dy), the
 *     centre included and treated like any other; q is skipped when outside the image, invalid or id[q] != id[p]:
 *       dn = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, clamped to [0, 1] (dn < 0 -> 0, then dn > 1 -> 1: a NaN
 *            stays), then squared normal_power_log2 times
 *       e = point[q] - point[p];  xz = |(n_p.x e.x + n_p.y e.y) + n_p.z e.z| / den_z
 *       xl = |lum(color[p]) - lum(color[q])| / den_l
 *       w = ((h[dy+2] h[dx+2]) dn) g(xz) g(xl), multiplied left to right
 *     a tap whose w is not > 0 is skipped (a NaN from an overflowed luminance or an underflowed denominator
 *     included); otherwise sw = sw + w;  sc[c] = sc[c] + w color[q][c];  sv2 = sv2 + (w w) variance[q]
 *   output: sw > 0: color'[p] = sc / sw, variance'[p] = sv2 / (sw sw); otherwise p passes through.
 * Out-of-image and invalid taps are skipped, never clamped.  g agrees with exp(-x) to second order at 0 and has a
 * heavier tail.
 *
 * kdpt_denoise_buffers is the filter alone on caller data on `device`: host arrays (3*w*h floats for color, normal,
 * point; w*h for variance, depth, id), w, h >= 1, w*h <= 2^26; out_color (3*w*h floats) and out_variance (w*h
 * floats, may be NULL) are host memory and must not alias the inputs.  Argument errors (a null pointer, w or h < 1,
 * w*h > 2^26, params out of range) are KDPT_ERR_ARG, reported before any device call.  It is what denoises data
 * that is not the context's image, a kdpt_trace_rays_moments bake for instance.
 *
 * kdpt_denoise is the same filter on the context's own render, defined as a composition:
 *   colour:   n_p = samples + extra[p] (samples while extra is absent);  color[p][c] = fdiv(image[p][c], (float)n_p)
 *   variance: v_c and vbar exactly as kdpt_noise_map spells them with n = n_p, in double, in that order;
 *             variance[p] = (float)(vbar / n).  This is the channel-mean variance beside the channel-mean
 *             luminance: a proxy for the variance of the luminance itself (an upper bound of it when the channels
 *             move together), not that variance.
 *   guides:   the camera's pinhole ray through every pixel -- from the eye, direction
 *             normalize(view - right pixelLength.x (x - W/2) - up pixelLength.y (y - H/2)), generateRayFromCamera's
 *             first part in its operation order, without jitter or lens whatever the context's options say (they are
 *             left alone) -- and for each ray the record kdpt_cast_rays(flags = 0) returns: normal, point,
 *             depth = t, id = material; depth = -1 where kind <= 0, so that pixel is invalid and passes through.
 *             (These are not the rays kdpt_camera_rays returns with antialias = 0 and dof_angle = 0: its lens
 *             arithmetic, (eye + d f) - d f and a second normalize, moves the last bit of some of them.)
 *             First-hit guides describe the surface, not what is seen in it: mirrors and glass are filtered as the
 *             surface they are.
 * Synchronous: waits for the work queued on the context (the pipelined adds included), runs on its stream, and
 * writes out_color (3*W*H floats) and out_variance (W*H floats, may be NULL), each host memory or memory of the
 * context's device, told apart as kdpt_write_pbo does.  It leaves the image, sumsq, samples, extra, kdpt_stats, the
 * pipeline slots, kdpt_cast_rays' buffers and counters and kdpt_trace_rays' state as they were.  Its buffers are
 * made on first use, owned by the context, freed by kdpt_destroy and remade after kdpt_set_tuning; the guides are
 * rebuilt on every call (no cache to invalidate).  Errors, reported before any device work: KDPT_ERR_ARG for a null
 * ctx, params or out_color, params out of range, or fewer than 2 uniform iterations accumulated;
 * KDPT_ERR_UNSUPPORTED while moments are off, and for contexts with enable_kd = 0 or viz_kd = 1 (kdpt_cast_rays'
 * own refusal).  kdpt_denoise_stats reports the last call's device times (hipEvents on the context's stream): the
 * guides (rays, traversal, hit records) and the filter (packing, the passes, the copy out). */
typedef struct kdpt_denoise_params {  /* 24 bytes */
    int passes, normal_power_log2;
    float sigma_l, sigma_z, eps_l, pad_;
} kdpt_denoise_params;
void kdpt_default_denoise_params(kdpt_denoise_params *p);
int kdpt_denoise_buffers(int device, int w, int h, const float *color, const float *variance, const float *normal,
                         const float *point, const float *depth, const int *id, const kdpt_denoise_params *p,
                         float *out_color, float *out_variance /* may be NULL */);
int kdpt_denoise(kdpt_ctx *ctx, const kdpt_denoise_params *p, float *out_color, float *out_variance /* may be NULL */);
int kdpt_denoise_stats(kdpt_ctx *ctx, double *guide_ms, double *filter_ms);

/* ---- Temporal accumulation: the denoiser's history, reprojected across views ----
 * SVGF's other half (Schied et al. 2017), for a camera that moves through a static scene: kdpt_set_camera, kdpt_reset,
 * a few iterations, and kdpt_denoise_temporal in place of kdpt_denoise.  The frame's colour and variance are blended
 * with the previous call's before the spatial filter sees them.  The scene does not move, so the world-space point of
 * every first hit -- already in the denoiser's guides -- is its own motion vector: a pixel projects its hit point
 * through the previous camera and accepts a history tap only when the tap lies on the same surface in world space.
 * The projection only proposes taps, the world-space tests accept them: a camera that is not orthonormal, or rounding
 * in fx, can cost history but never mix surfaces.
 * Like "Denoising" the contract is a bit pattern: float32 add, subtract, multiply, divide, compare, abs, floorf and
 * float -> int conversion only, every operation rounded on its own (no fused multiply-add), denormals kept, so a
 * numpy float32 restatement gives the same bits.
 *
 * Current frame, W x H, pixel p = y*W + x: color C[p][3], variance V[p] (of the pixel's mean), normal n_p, point X_p,
 * depth_p, id_p; p is valid by "Denoising"'s rule (its 11 floats finite, depth > 0, variance >= 0).
 * History (absent, or the previous call's): the same six quantities and a length L[q] (float, >= 0: how many frames
 * the pixel has accumulated), and the camera cam' they were made under.  A history pixel q is usable iff
 * depth[q] > 0 and L[q] > 0 (nothing else is asked of it: its colour and variance enter as they are).
 *
 * kdpt_temporal_params (kdpt_default_temporal_params fills the defaults, chosen by eye): alpha in (0, 1] (0.2);
 * sigma_z > 0 (0.02); normal_min in [-1, 1] (0.9); max_history 1 .. 4096 (32); the floats finite.
 *
 * An invalid pixel passes through, C' = C, V' = V, and stores L' = 0.  A valid pixel p, in this order:
 *   projection: e = X_p - cam'.position;  z = (e.x v.x + e.y v.y) + e.z v.z with v = cam'.view;  a and b the same
 *     dot product with cam'.right and cam'.up.  No history if !(z > 0).
 *     fx = W 0.5f - (a / z) / pixelLength.x;  fy = H 0.5f - (b / z) / pixelLength.y  (the inverse of the guides'
 *     pinhole direction: pixel x is the centre of its own ray, no half-pixel offset).
 *     No history if !(fx > -1 && fx < W && fy > -1 && fy < H).
 *     ix = (int)floorf(fx), tx = fx - floorf(fx);  iy, ty likewise.
 *   taps: q = (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) in that order, w = wx wy with wx = 1 - tx or tx and
 *     wy = 1 - ty or ty.  A tap is skipped when it is outside the image, when q is not usable, when id[q] != id_p,
 *     when !((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_min), when, with d = X_q - X_p,
 *     !(|(n_p.x d.x + n_p.y d.y) + n_p.z d.z| / (sigma_z depth_p) <= 1), or when !(w > 0); a NaN anywhere in these
 *     therefore rejects the tap.  Otherwise sw = sw + w;  sc[c] = sc[c] + w C_h[q][c];  sv = sv + w V_h[q];
 *     sl = sl + w L[q].
 *   blend: !(sw > 0): no history, C' = C, V' = V, L' = 1, bit for bit.  Otherwise h = sc / sw, vh = sv / sw,
 *     lh = sl / sw;  l = lh + 1;  L' = l < (float)max_history ? l : (float)max_history;  r = 1 / L';
 *     A = r > alpha ? r : alpha;  B = 1 - A;
 *     C'[c] = fadd(fmul(B, h[c]), fmul(A, C[c]));  V' = fadd(fmul(fmul(B, B), vh), fmul(fmul(A, A), V)).
 * The blend is a weighted sum of independent frame means, so its variance is the squared-weight sum: the stage
 * carries the variance itself, not luminance moments.  V_h is resampled with weight w, not w^2 (the variance of the
 * interpolated history would be smaller): deliberately conservative.
 *
 * kdpt_temporal_buffers is the stage alone on caller data on `device`, with kdpt_denoise_buffers' conventions: host
 * arrays (3*w*h floats for color, normal, point; w*h for variance, depth, id, length), w, h >= 1, w*h <= 2^26;
 * out_color (3*w*h floats), out_variance and out_length (w*h floats each) are host memory, all required, and must
 * not alias the inputs.  The eight history arguments (seven arrays and h_camera) are all NULL -- no history -- or all
 * given; h_camera->resolution must be (w, h).  Argument errors (a null pointer, a history given in part, w or h < 1,
 * w*h > 2^26, params out of range or not finite, a resolution mismatch) are KDPT_ERR_ARG, reported before any device
 * call.
 *
 * kdpt_denoise_temporal is a composition, with temporal() the stage above and filter() "Denoising"'s passes:
 *   C, V and the guides G are exactly what kdpt_denoise derives from the context's current state;
 *   (C', V', L') = temporal(C, V, G; history, history camera);
 *   history := (C', V', L', G) and the context's current camera;
 *   output = filter(C', V', G, dp); dp->passes = 0 gives the temporal stage's output itself.
 * With no history the result is kdpt_denoise's, bit for bit.  Synchronous, on the context's stream, out_color and
 * out_variance (may be NULL) host memory or memory of the context's device, as kdpt_denoise's; it leaves alone
 * everything kdpt_denoise leaves alone, and the only state it changes is the history.  The history is owned by the
 * context, made on first use: two sets of 52 bytes per pixel (three 16-byte records and the length; the frame is
 * built in one while the other is read, and the two swap roles), 104 bytes per pixel beside kdpt_denoise's buffers.
 * It survives kdpt_reset, kdpt_set_camera and kdpt_set_options -- a frame of a camera path is "set camera, reset,
 * trace, denoise" -- and is dropped by kdpt_temporal_reset, by kdpt_set_tuning (with the denoiser's other buffers)
 * and by kdpt_destroy.  Errors are kdpt_denoise's, plus KDPT_ERR_ARG for a null or out-of-range tp; they are
 * reported before any device work and leave the history untouched.
 * kdpt_temporal_stats reports the last call: three device times (hipEvents on the context's stream: the guides; the
 * packing and the temporal stage; the passes and the copy out) and two counts, the frame's valid pixels and those
 * of them that found history (sw > 0). */
typedef struct kdpt_temporal_params {  /* 24 bytes */
    float alpha, sigma_z, normal_min;
    int max_history;
    float pad_[2];
} kdpt_temporal_params;
void kdpt_default_temporal_params(kdpt_temporal_params *p);
int kdpt_temporal_buffers(int device, int w, int h,
                          const float *color, const float *variance, const float *normal, const float *point,
                          const float *depth, const int *id,
                          const float *h_color, const float *h_variance, const float *h_normal, const float *h_point,
                          const float *h_depth, const int *h_id, const float *h_length,
                          const kdpt_camera *h_camera, const kdpt_temporal_params *p,
                          float *out_color, float *out_variance, float *out_length);
int kdpt_denoise_temporal(kdpt_ctx *ctx, const kdpt_temporal_params *tp, const kdpt_denoise_params *dp,
                          float *out_color, float *out_variance /* may be NULL */);
int kdpt_temporal_reset(kdpt_ctx *ctx);
int kdpt_temporal_stats(kdpt_ctx *ctx, double *guide_ms, double *temporal_ms, double *filter_ms,
                        long long *valid, long long *with_history);

/* ---- A persistent group: the in-process sharded renderer as an object ----
 * kdpt_render_sharded's contexts kept alive: one context per device in this process, created once (scene upload
 * and mask tables once per rank), rendering frames call after call, and, with KDPT_GROUP_MOMENTS, carrying second
 * moments through the cross-rank reduce, so that the noise estimate and adaptive sampling work on the sharded
 * deployment.  kdpt_render_sharded is kdpt_group_create, kdpt_group_render_frames, kdpt_group_synchronize and
 * kdpt_group_destroy.
 *
 * kdpt_group_create takes kdpt_render_sharded's arguments and rules: ndev 1 .. 8 contexts on devices[0 .. ndev), a
 * device may repeat with KDPT_REDUCE_COPY, opt->external_image is ignored, RCCL is loaded at run time
 * (KDPT_ERR_UNSUPPORTED when it is absent).  KDPT_ERR_ARG, reported before any device work as kdpt_create reports
 * its own, for a null scene, devices or out, ndev outside 1 .. 8, a reduce that is neither KDPT_REDUCE_*, or an
 * unknown flag bit; a scene kdpt_create refuses is refused with kdpt_create's code and message, before any device
 * work too.  A failure part-way releases everything already made and leaves *out NULL.  The group owns its contexts,
 * the copy reduce's staging buffers, the events recorded across devices and the communicators;
 * kdpt_group_destroy(NULL) is KDPT_OK.
 * flags = KDPT_GROUP_MOMENTS: every rank's frame buffers hold S and Q (6*W*H floats, S first, one allocation, so
 * one reduce moves both) and rank 0's context has moments on (kdpt_set_moments): it keeps sumsq, the sample counter
 * and, from the first adaptive call on, extra.  Device memory per rank: 2 x 6*W*H floats of frame buffers in
 * place of 2 x 3*W*H (and rank 0's reduced frame and the copy reduce's staged parts likewise), plus W*H ints for an
 * adaptive round's list on every rank but the first.
 *
 * kdpt_group_render_frames queues frames first_frame .. first_frame + frames - 1 and returns; frames, shares and
 * the reduce are kdpt_render_sharded's (frame f = global iterations f*spp + 1 .. (f+1)*spp, rank r those with
 * (iteration - 1 - f*spp) % N == r, two frame buffers in flight, `out` as there: host or rank 0's device memory,
 * frames * 3*W*H floats, or NULL; a pageable host `out` stays pinned until kdpt_group_synchronize and must stay
 * allocated until it returns).  kdpt_group_synchronize waits for every rank, checks every rank's fault words
 * (every rank is drained even when one reports a fault; the first failure is returned) and releases the pinned
 * `out`.  Without KDPT_GROUP_MOMENTS rank 0's image and `out` are bit-equal to kdpt_render_sharded's for the same
 * arguments.  A later call continues on the same contexts: its frames add into rank 0's image in frame order, so
 * frames 0-1 then 2-3 give the image of frames 0-3 in one call, bit for bit.
 *
 * Frames with second moments (KDPT_GROUP_MOMENTS).  Rank r's iterations of the frame i1 < i2 < ... (global
 * numbers, stride N), x an iteration's partial value, from a zeroed buffer and in iteration order:
 *   S_r = fadd(S_r, x);  Q_r = fadd(Q_r, fmul(x, x))
 * (two roundings for Q, never a fused multiply-add, as kdpt_set_moments spells for sumsq).  One reduce over 6*W*H
 * floats: the copy reduce adds the ranks in rank order, S_f = (S_0 + S_1) + ..., Q_f likewise; RCCL runs one
 * ncclReduce (its order); a rank without an iteration in the frame contributes zeros.  Rank 0 then, per frame and
 * in one pass: image = fadd(image, S_f), sumsq = fadd(sumsq, Q_f), samples += spp.  `out` receives S_f alone; Q is
 * read with kdpt_read_moments on rank 0's context.  The image's bits are those of the same group without the flag.
 * As frames against kdpt_trace_iterations, this is not the bit pattern of one context that adds every iteration
 * into its image: partial sums are added once per frame.
 *
 * kdpt_group_context lends rank `rank`'s context (borrowed: the group still owns it) for calls that leave the
 * render state alone: kdpt_read_image, kdpt_read_moments, kdpt_noise_map, kdpt_noise_estimate,
 * kdpt_read_sample_counts, kdpt_save_*, kdpt_get_stats, kdpt_cast_rays, kdpt_trace_rays[_moments],
 * kdpt_camera_rays, kdpt_denoise, kdpt_denoise_temporal and kdpt_temporal_reset (rank 0 of a KDPT_GROUP_MOMENTS
 * group: the sharded render denoised; the history is the only state they change).  They see the
 * frames queued so far (rank 0's reads follow the group's last image add without
 * a kdpt_group_synchronize; fault words are checked only there).  A borrowed context must not receive
 * kdpt_destroy, nor a call that changes its state: kdpt_trace_iteration[s][_async], kdpt_render_frames,
 * kdpt_trace_adaptive, kdpt_active_pixels, kdpt_reset, kdpt_set_moments, kdpt_set_options, kdpt_set_camera,
 * kdpt_set_tuning, kdpt_comm_init -- the kdpt_group_* calls are their counterparts.
 *
 * kdpt_group_set_camera and kdpt_group_set_options validate once (kdpt_set_camera's and kdpt_set_options' rules)
 * and apply to every rank, or, on a refusal, to none; kdpt_group_set_options waits for the queued work first.
 * kdpt_group_reset waits and resets every rank (rank 0's image, sumsq, samples and extra are zero afterwards).
 *
 * Adaptive rounds (KDPT_GROUP_MOMENTS; KDPT_ERR_UNSUPPORTED without it).  extra[p] lives on rank 0, made on first
 * use, zeroed by kdpt_group_reset.  kdpt_group_active_pixels returns the list A kdpt_active_pixels would build from
 * rank 0's image, sumsq, samples and extra: the same kernels and the same rule, ascending.
 * kdpt_group_trace_adaptive is synchronous: it synchronises the group, builds A on rank 0, reads |A| back once,
 * copies the list to every other rank's device, and gives iteration first_iter + k (k < count) to rank k mod N.
 * Each rank runs its iterations over A on the batched, pipelined route (path j = the camera's ray of that
 * iteration through pixel A[j], pixelIndex j, as in kdpt_trace_adaptive) and accumulates them in order, from a
 * zeroed buffer of 6 |A| floats: s_r[j] = fadd(s_r[j], x), q_r[j] = fadd(q_r[j], fmul(x, x)).  The slot buffers
 * are reduced as frames are (rank order for the copy reduce), and rank 0 does, for every slot j and channel,
 *   image[A[j]] = fadd(image[A[j]], s[j]);  sumsq[A[j]] = fadd(sumsq[A[j]], q[j]);  extra[A[j]] += count.
 * The partial sums are added once per round, not once per iteration, so the result is NOT the bit pattern of
 * kdpt_trace_adaptive on one context (as frames are not kdpt_trace_iterations'); it does not depend on pipeline
 * or batch.  `out` is filled as kdpt_trace_adaptive fills it, segments and traced summed over the ranks,
 * device_ms rank 0's (from after the list to after the round's add).  With |A| = 0 or count = 0 nothing changes;
 * the uniform `samples` counter and every rank's kdpt_stats do not move.  Errors are kdpt_trace_adaptive's (a
 * null group for its null ctx), reported before any device work; the single-context calls keep refusing a
 * context that is in a communicator. */
typedef struct kdpt_group kdpt_group;
#define KDPT_GROUP_MOMENTS 1   /* every rank carries second moments; rank 0 keeps sumsq, samples, extra */
int kdpt_group_create(const kdpt_scene *scene, const kdpt_options *opt, int ndev, const int *devices,
                      int reduce, int flags, kdpt_group **out);
int kdpt_group_render_frames(kdpt_group *g, int first_frame, int frames, int spp, int pipeline, int batch, float *out);
int kdpt_group_synchronize(kdpt_group *g);
int kdpt_group_context(kdpt_group *g, int rank, kdpt_ctx **ctx);   /* borrowed */
int kdpt_group_active_pixels(kdpt_group *g, float floor, float threshold, int *pixels, long long *n);
int kdpt_group_trace_adaptive(kdpt_group *g, int first_iter, int count, int pipeline, int batch,
                              float floor, float threshold, kdpt_adaptive *out);
int kdpt_group_set_camera(kdpt_group *g, const kdpt_camera *camera);
int kdpt_group_set_options(kdpt_group *g, const kdpt_options *opt);
int kdpt_group_reset(kdpt_group *g);
int kdpt_group_destroy(kdpt_group *g);

int kdpt_destroy(kdpt_ctx *ctx);
/* The message of the most recent failing call of any kdpt_* function on the calling thread (each thread has its
 * own; "" before the first failure).  A successful call leaves it alone, so read it only after a non-OK return.
 * The pointer is valid until that thread's next failing call. */
const char *kdpt_last_error(void);

/* Device pointer of the accumulation image (for an in-place RCCL reduce). */
int kdpt_image_device_ptr(kdpt_ctx *ctx, void **dptr);
/* Debug / parity: run iteration `iter` through bounce `stop_depth` (0-based) and copy the
 * live PathSegment array (reference layout) to host `out` (>= W*H entries). */
int kdpt_debug_paths(kdpt_ctx *ctx, int iter, int stop_depth, kdpt_path_segment *out, int *npaths);
/* Roofline counters: one extra, untimed iteration that also counts AABB tests, triangle
 * tests and triangle hits (aabb_tri_hit[3]); the image is not touched.  Afterwards kdpt_get_stats
 * reports that iteration's segments and seg_per_bounce. */
int kdpt_count_iteration(kdpt_ctx *ctx, int iter, unsigned long long *aabb_tri_hit);
/* Of the last kdpt_count_iteration: the AABB tests done before the intersect kernel (the root-box test of
 * the rays that miss the KD root, made by k_geoms / the previous bounce's shading pass) and the number of
 * ray segments handed to the intersect kernel (aabb_prep_cand[2]). */
int kdpt_count_split(kdpt_ctx *ctx, unsigned long long *aabb_prep_cand);
/* Diagnostic: cycle profile of the intersect kernel during the last kdpt_count_iteration.
 * Copies up to n values -- node trips, node cycles, big-leaf sweeps, big-leaf cycles,
 * small-leaf phases, small-leaf rounds, small-leaf cycles, recombination cycles, setup
 * cycles, analytic-geometry cycles, post cycles, node lane-steps, big leaves swept, their
 * clusters, clusters tested with a u/v pass, ... with several, small-leaf (ray, triangle) pairs,
 * node-trip lanes waiting on a leaf, ... finished, cycles after the ray queue ran dry, finished
 * node-trip lanes then (each summed over waves), waves, wave cycles, aabb, tri, hit, then a 64-bin
 * histogram of intersect-wave lifetimes
 * (10 us bins), a 64-bin histogram of node steps per ray (bins of 4), and node steps summed / rays counted
 * by the ray's chord through the KD root box (8 bins, eighths of its diagonal) -- and returns how many exist. */
int kdpt_wave_profile(kdpt_ctx *ctx, unsigned long long *out, int n);
/* Device-math known answers: sinf/cosf/pow-5 Fresnel/u01 evaluated by the gfx950 code. */
int kdpt_selftest_math(const float *x, int n, float *sin_out, float *cos_out);
int kdpt_selftest_rng(const int *iter_idx_depth, int n, int k, float *u_out);
/* The first k uniform draws (n x k) of thrust::default_random_engine + uniform_real_distribution<float>
 * as the device restates them, per input: mode 0 makeSeededRandomEngine(iter, index, depth) of int
 * triples (src/pathtrace.cu:62-66), 1 the camera jitter's engine(utilhash(iter)) (src/pathtrace.cu:334),
 * 2 engine(seed) of raw uint32 seeds.  Pinned to rocThrust by tests/golden/ref_pins.json. */
int kdpt_selftest_rng_draws(int mode, const uint32_t *in, int n, int k, float *out);
int kdpt_selftest_fresnel(const float *cosines, int n, float ior, float *f_out);
/* The glm pieces on the path (kdpt_glm_kat.h glm_kat, vendored glm 0.9.6.3 restated): fn 0
 * intersectRayTriangle (15 floats in -> {passed, bary.xyz}; `out` holds sentinels on entry, kept where
 * glm leaves bary unwritten), 1 normalize (3 -> 3), 2 reflect (6 -> 3), 3 refract (7 -> 3),
 * 4 glm::rotate(quat, vec3) (7 -> 3).  Run on the device. */
int kdpt_selftest_glm(int fn, const float *in, int n, float *out);
/* The bounce as units, run on the device, one record of 32-bit words per lane (float unless said otherwise;
 * csrc/kdpt_bounce_kat.h).  scatter: scatterRay (src/interactions.h:195-358) with engine(seed) -- in: origin 0-2,
 * direction 3-5, isinside 6 (0 / 1), sdepth 7, intersect 8-10, normal 11-13, hasReflective 14, hasRefractive 15,
 * indexOfRefraction 16, transmittance 17-19, softness 20, seed 21 (uint32); out: origin 0-2, direction 3-5,
 * isinside 6, sdepth 7, the engine's next u01 draw 8.  shade: shadeMaterial's body (src/pathtrace.cu:2318-2366)
 * -- in: t 0, colour 1-3, specular colour 4-6, hasReflective 7, hasRefractive 8, emittance 9, transmittance
 * 10-12, enable_sss 13 (0 / 1), sdepth 14, path colour 15-17, remainingBounces 18 (int32); out: path colour 0-2,
 * remainingBounces 3 (int32). */
int kdpt_selftest_scatter(const float *in, int n, float *out);
int kdpt_selftest_shade(const float *in, int n, float *out);
/* The scatter's glibc calls as restated for gfx950 (src/interactions.h:67-83,214): fn 0 acosf(x),
 * 1 sin((double)x), 2 cos((double)x); results as doubles. */
int kdpt_selftest_libm(int fn, const float *x, int n, double *out);
/* Order-independent digest of fn over the float bit patterns first .. first+count-1 (count <= 2^32):
 * sum mod 2^64 of splitmix64(result bits ^ splitmix64(input bits)); the oracle's orc_libm_digest
 * computes the same with the host glibc. */
int kdpt_selftest_libm_digest(int fn, uint32_t first, unsigned long long count, unsigned long long *digest);

/* ---- Host scene building (C++ restatement of the reference's host code) ---- */
typedef struct kdpt_scene_data kdpt_scene_data;

/* Scene text (src/scene.cpp:7-271) + optional OBJ (src/scene.cpp:579-968, tinyobjloader)
 * + the runCuda camera (src/main.cpp:1059-1073,1111-1129).  Overrides <= 0 keep the file
 * values; a resolution override recomputes pixelLength with the loadCamera formula. */
int kdpt_scene_load(const char *scene_path, const char *obj_path, int res_w, int res_h, int depth,
                    kdpt_scene_data **out);

/* kdpt_scene_load with the KD tree built on GPU `device` (byte-identical; see kdpt_scene_build_device). */
int kdpt_scene_load_device(const char *scene_path, const char *obj_path, int res_w, int res_h, int depth,
                           int device, kdpt_scene_data **out);

/* The same from already-parsed values (what the parsers produce; fixtures use this). */
typedef struct kdpt_scene_desc {
    int res[2];
    float fovy;
    int iterations;
    int traceDepth;
    float eye[3], lookAt[3], up[3];
    int num_materials;
    const kdpt_material *materials;
    int num_geoms;
    const int *geom_type;
    const int *geom_material;
    const float *geom_trs;          /* per geom: translation[3], rotation[3], scale[3] */
    int ntri;                       /* 0: no OBJ */
    const float *verts9, *norms9;   /* per triangle, vertex-index-gathered normals */
    const int *shape_of_tri;
    int num_shapes;
    const kdpt_material *shape_materials;
    int kd_max_depth;               /* 0 = 13, the reference's split(13) */
} kdpt_scene_desc;
int kdpt_scene_build(const kdpt_scene_desc *desc, kdpt_scene_data **out);
/* The same, with the KD tree built on GPU `device` (csrc/kd_build.hip: level by level, breadth first, then
 * pre-order IDs) instead of the host recursion; the arrays are byte-identical to kdpt_scene_build's
 * (KDnode::split src/KDnode.cpp:151-249, Scene::loadObj src/scene.cpp:866-968). */
int kdpt_scene_build_device(const kdpt_scene_desc *desc, int device, kdpt_scene_data **out);
/* Wall time of the GPU KD build of a kdpt_scene_build_device scene (0 for a host build). */
int kdpt_scene_kd_build_ms(const kdpt_scene_data *sd, double *ms);
/* The GPU KD build alone over a triangle soup (9 vertex + 9 normal floats and an mtlIdx per triangle, the
 * reference's Triangle order): NodeBare[] in ID order and TriBare[] in leaf order, malloc'd (kdpt_free). */
int kdpt_build_kd_device(const float *verts9, const float *norms9, const int *mtl, int ntri, int maxdepth,
                         int device, kdpt_node_bare **nodes, int *nnodes, kdpt_tri_bare **tris, int *ntris,
                         double *ms);
/* View of the built scene as the C-ABI struct (pointers owned by the scene data). */
int kdpt_scene_view(const kdpt_scene_data *sd, kdpt_scene *out);
int kdpt_scene_free(kdpt_scene_data *sd);

#ifdef __cplusplus
}
#endif
#endif /* KDPT_H */
