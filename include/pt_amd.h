/*
 * pt_amd.h -- C ABI of the MI355X-native path-tracing hot path (libpt_amd.so).
 *
 * Drop-in boundary for CIS565-Fall-2015/Project3-CUDA-Path-Tracer's renderer API
 *     void pathtraceInit(Scene *scene);                       reference src/pathtrace.h:6,  src/pathtrace.cu:75-85
 *     void pathtraceFree();                                   reference src/pathtrace.h:7,  src/pathtrace.cu:87-92
 *     void pathtrace(uchar4 *pbo, int frame, int iteration);  reference src/pathtrace.h:8,  src/pathtrace.cu:123-174
 * Those three symbols are C++-mangled and take a libstdc++/glm-dependent `Scene*`, so the FFI-able
 * core below takes plain pointers and sizes; the ~40-line C++ shim that provides the three reference
 * symbols on top of it is project3-cuda-path-tracer_amd/host/pathtrace_shim.cpp.
 *
 * PtGeom / PtMaterial / PtCamera are byte-identical to Geom / Material / Camera of reference
 * src/sceneStructs.h:18-47, so `scene->geoms.data()`, `scene->materials.data()` and
 * `&scene->state.camera` pass straight through.
 *
 * All functions return PT_OK (0) or a negative PtStatus; pt_last_error() describes the calling thread's last failure.
 * A renderer instance is a CONTEXT.  The functions below act on the calling thread's CURRENT context: the process-wide default one --
 * one renderer per process, like the reference's file-static state (src/pathtrace.cu:70-71) -- unless pt_ctx_make_current named another
 * (section "contexts and device groups" at the end: several renderers in one process, one per device of a node).  One context is driven by
 * one host thread at a time (the reference is single-threaded); different threads may drive different contexts.
 */
#ifndef PT_AMD_H
#define PT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtVec3 { float x, y, z; } PtVec3;

/* reference src/sceneStructs.h:8-11; PT_MESH: the third object type of the scene format (README.md:236, "mesh"), which the
 * reference's enum and loader do not have -- see pt_set_meshes */
enum { PT_SPHERE = 0, PT_CUBE = 1, PT_MESH = 2 };

/* reference src/sceneStructs.h:18-27 -- 236 bytes, mat4 column-major (m[col*4+row]) */
typedef struct PtGeom {
    int32_t type;
    int32_t materialid;
    PtVec3  translation, rotation, scale;
    float   transform[16];
    float   inverseTransform[16];
    float   invTranspose[16];
} PtGeom;

/* reference src/sceneStructs.h:29-39 -- 44 bytes (flags are floats) */
typedef struct PtMaterial {
    PtVec3 color;
    float  specularExponent;
    PtVec3 specularColor;
    float  hasReflective, hasRefractive, indexOfRefraction, emittance;
} PtMaterial;

/* reference src/sceneStructs.h:41-47 -- 52 bytes; fov in degrees, fov.y = vertical HALF angle */
typedef struct PtCamera {
    int32_t resolution[2];
    PtVec3  position, view, up;
    float   fov[2];
} PtCamera;

typedef enum PtStatus {
    PT_OK = 0,
    PT_ERR_INVALID = -1,      /* bad argument */
    PT_ERR_NOT_INIT = -2,     /* pt_iterate & co. before pt_init */
    PT_ERR_HIP = -3,          /* a HIP runtime call failed (replaces checkCUDAError, pathtrace.cu:21-39) */
    PT_ERR_DEVICE = -4,       /* a kernel reported an internal fault (path pool exhausted, chunk-list timeout): sticky,
                                 reported by pt_sync / pt_counters; results void */
    PT_ERR_NO_GPU = -5        /* no HIP device: there is NO CPU fallback */
} PtStatus;

enum {
    PT_FLAG_KERNEL_TIMING = 1,   /* bracket every bounce-kernel launch with HIP events (roofline measurement) */
    PT_FLAG_ACCUM_SHARD_ROWS = 2,/* the accumulator holds ONLY this shard's rows, packed (local row lr = global row
                                    lr * shard_count + shard_rank; nLocal * 3 floats): what a multi-GPU run gathers
                                    at rank 0 instead of reducing zero-padded full frames.  pt_readback still returns
                                    a full frame (other rows zero). */
    PT_FLAG_TRACE_AHEAD = 8,     /* for callers that keep the reference's protocol -- pathtrace(pbo, frame, iter) once per iteration
                                    with iter = 1, 2, 3, ... (src/main.cpp:97-103): pt_iterate(frame, iter) traces iterations
                                    iter .. iter + max_batch - 1 as ONE wavefront batch (iterations are independent: RNG keyed on
                                    iteration / pixel / depth), commits iteration `iter` alone and parks the radiance of the others;
                                    the calls for iter + 1, iter + 2, ... then only commit theirs, while the free slots of the
                                    pipeline trace the batches that follow.  The accumulator after every call is bit-identical to
                                    the one without the flag.  A call that does not continue the sequence (another iter, a
                                    pt_iterate_batch with count > 1) discards what is parked and starts over; pt_init / pt_free
                                    discard as well (the reference's camera-move restart, src/main.cpp:91-95).  Needs max_batch > 1
                                    to have any effect.  PtCounters: `iterations` counts committed iterations; live / light_hits /
                                    misses also cover the iterations traced ahead. */
    PT_FLAG_MIXTURE_WEIGHTED = 16,/* A material with REFL > 0 scatters 50 / 50 between the mirror and the diffuse lobe.  The reference's comment asks
                                    for "a 50/50 split ... divided by the probability" (src/interactions.h:54-58); the build's default
                                    takes SURVEY S6's energy-conserving reading WITHOUT the 1 / p weight, because that is what the
                                    staff render shows (the weighted form is 1.32 x on Cornell's back wall).  This flag renders the
                                    documented reading: the branch taken carries its weight 2 (the oracle's mirror mode 1). */
    PT_FLAG_MOMENTS = 32,        /* the renderer also keeps, per pixel, the sum of its samples' squared luminance (one more device buffer of W*H
                                    floats, always the library's own): every commit adds l * l, l = (0.2126 r + 0.7152 g) + 0.0722 b of the sample
                                    it adds to the accumulator, in the same iteration order.  What pt_readback_moments, pt_variance and
                                    pt_denoise_var need.  The accumulator is bit-identical to the one without the flag.  PT_ERR_INVALID with
                                    shard_count > 1 or PT_FLAG_ACCUM_SHARD_ROWS, and from pt_group_init. */
    PT_FLAG_TEMPORAL = 64,       /* temporal reprojection (section "temporal reprojection" below): a pt_init over the LIVE renderer of the same context
                                    -- no pt_free in between -- keeps the old view's colour, second moment and sample count per pixel as the
                                    context's HISTORY, and pt_denoise_var / pt_denoise_var_rgba8 of the new renderer filter the count-weighted blend
                                    of that history, reprojected, with the new samples.  Nothing else reads it: both accumulators, pt_variance,
                                    pt_noise_stats, pt_iterate_until, pt_readback* and pt_denoise are the unflagged renderer's bit for bit, and so is
                                    pt_denoise_var while the context holds no history.  PT_ERR_INVALID without PT_FLAG_MOMENTS, with
                                    PT_FLAG_TRACE_AHEAD, and with lens_radius > 0 (a thin lens has no single projection). */
    PT_FLAG_DISPLAY_FILTER = 128,/* the display filter (section "display filter" below): every call that writes sendImageToPBO's bytes of the
                                    accumulator -- pt_iterate / pt_iterate_batch with rgba8_dev != NULL, pt_readback_rgba8 -- writes the bytes
                                    pt_denoise_var_rgba8 with the PT_DISPLAY_* setting would return at that point of the stream, on the device and
                                    without a synchronisation.  Everything else is the unflagged renderer's bit for bit.  PT_ERR_INVALID without
                                    PT_FLAG_MOMENTS, and for a scene whose guide buffers cannot be made. */
    PT_FLAG_SPATIAL_VARIANCE = 256,/* the spatial variance estimate (section "spatial variance" below): pt_denoise_var / pt_denoise_var_rgba8 accept
                                    samples == 1, and a pixel whose effective sample count is below PT_SPATIAL_MIN_COUNT -- which has no variance of
                                    its own -- is filtered under a variance estimated from its neighbours' luminance moments; with
                                    PT_FLAG_DISPLAY_FILTER the display's first frame is filtered too.  From two samples on everything is the
                                    unflagged renderer's bit for bit, launch for launch.  PT_ERR_INVALID without PT_FLAG_MOMENTS. */
    PT_FLAG_DEMODULATE = 512,    /* albedo demodulation (section "demodulation" below): the renderer also keeps, per pixel, the sum of the first-hit
                                    albedo of every committed iteration's camera ray (one more device buffer of W*H float4, always the library's
                                    own), and pt_denoise_var / pt_denoise_var_rgba8 -- under PT_FLAG_DISPLAY_FILTER the display path too -- divide
                                    the pixel's mean albedo out in front of the filter's levels and multiply it back behind them.  Everything else
                                    is the unflagged renderer's bit for bit.  PT_ERR_INVALID without PT_FLAG_MOMENTS, with PT_FLAG_TEMPORAL, with
                                    PT_FLAG_TRACE_AHEAD, and for a scene whose guide buffers cannot be made. */
    PT_FLAG_DEMOD_HISTORY = 1024,/* history carries albedo (section "demodulated history" below): with PT_FLAG_MOMENTS, PT_FLAG_TEMPORAL and
                                    PT_FLAG_DEMODULATE -- all three, which pt_init accepts together under this flag alone -- the context's history
                                    also keeps the old view's mean first-hit albedo per pixel, and pt_denoise_var / pt_denoise_var_rgba8 / the
                                    display path divide the blend of the reprojected history with the new samples by the BLENDED albedo.  While the
                                    context holds no history the renderer is PT_FLAG_DEMODULATE's bit for bit.  PT_ERR_INVALID without any of the
                                    three; every other refusal of PT_FLAG_TEMPORAL and of PT_FLAG_DEMODULATE stands. */
    PT_FLAG_KEEP_RENDERER = 2048,/* a flag about COST alone, for callers that repeat the full pt_init whenever the camera moves (the reference's
                                    Free -> Init restart, src/main.cpp:91-95; host/pathtrace_shim.cpp under PT_AMD_KEEP_RENDERER).  A full call
                                    that carries it over a LIVE renderer of the same context is compared with what that renderer was initialised
                                    with, and takes the same-scene form's path (PT_SAME_SCENE below: every buffer, stream and event kept) when all
                                    of these are equal: ngeoms and the geoms' bytes; nmats and the materials' bytes; traceDepth; every field of
                                    PtOptions, this flag included (stream, accum_dev and device as values); the camera's resolution; and what is
                                    registered NOW with pt_set_meshes / pt_set_textures / pt_set_bump_maps against the renderer's own copies --
                                    counts, sizes and bindings, the triangle, normal, face-material and UV arrays, and the texels, all byte for
                                    byte (memcmp, no hash).  In every other case -- a renderer initialised without the flag included: the flags
                                    differ -- the call is the full call it is today.  Either way the result is the full call's bit for bit (the
                                    same-scene form's own definition: accumulators, moments and albedo sums zeroed, counters reset, parked batches
                                    discarded, guide buffers invalidated, under PT_FLAG_TEMPORAL the old view captured into the history first),
                                    every refusal of the full call stands and happens before anything is touched, and a renderer with a sticky
                                    device fault, or a HIP failure before anything is overwritten, runs the full call inside.  Otherwise inert: a
                                    flagged renderer allocates and launches exactly what an unflagged one does, pt_free is unchanged, and an
                                    unflagged caller sees nothing new.  PT_ERR_INVALID from pt_group_init (groups re-initialise in place already).
                                    (Additive, no new function, no struct changed: the ABI version stays.) */
    PT_FLAG_OBJECT_HISTORY = 4096,/* history follows moved objects (section "object history" below): with PT_FLAG_MOMENTS and PT_FLAG_TEMPORAL.
                                    Between two renderers that both carry it the history passes a pt_init only when the old and the new scene
                                    describe the same objects -- ngeoms, every geom's type and materialid, nmats and the materials' bytes, and
                                    what is registered, byte for byte -- and is dropped otherwise: the caller's promise becomes a check.  The
                                    geoms' poses may differ: the reprojection then goes through each primitive's own motion.  PT_ERR_INVALID
                                    without either of the two flags, and from pt_group_init; every refusal of PT_FLAG_TEMPORAL stands.  A
                                    renderer without the flag is what it was in every respect.  (Additive, no new function, no struct changed:
                                    the ABI version stays.) */
    PT_FLAG_MOTION = 8192,       /* motion blur (section "motion blur" below): `geoms` of a full pt_init holds PT_MOTION_STEPS x ngeoms records,
                                    the scene in 16 poses across the shutter, and iteration i renders the pose PT_MOTION_STEP(i) alone.
                                    PT_ERR_INVALID with PT_FLAG_TEMPORAL, PT_FLAG_OBJECT_HISTORY, PT_FLAG_DISPLAY_FILTER, PT_FLAG_DEMODULATE,
                                    PT_FLAG_SPATIAL_VARIANCE or PT_FLAG_KEEP_RENDERER, and from pt_group_init.  A renderer without the flag is
                                    what it was in every respect.  (Additive, no new function, no struct changed: the ABI version stays.) */
    PT_FLAG_DIRECT_LIGHTING = 4/* README.md:107-108: "a final ray directly to a random point on an emissive object": at the
                                    last of the traceDepth bounces a diffuse scatter aims at a uniformly chosen point of a
                                    uniformly chosen emissive primitive (cosine-weighted), and ONE more bounce collects what
                                    that ray hits (traceDepth + 1 launches; traceDepth <= PT_MAX_DEPTH - 1).  A mesh is an
                                    emissive primitive when its object's material or ANY of its faces' materials emits; the
                                    point is drawn in the object-space bounding box of ALL its vertices either way.  At
                                    most 8 emissive primitives: pt_init refuses a scene with more under this flag
                                    (PT_ERR_INVALID) rather than choose among the first eight alone */
};

typedef struct PtOptions {
    int32_t shard_rank;       /* this process renders image rows y with y % shard_count == shard_rank */
    int32_t shard_count;      /* 1 = whole frame (reference behaviour) */
    int32_t device;           /* HIP device ordinal; -1 = current device */
    int32_t flags;            /* PT_FLAG_* */
    int32_t pipeline_depth;   /* iterations kept in flight on internal streams: 0 = default (3), 1 = none, max 4.
                                 Results do not depend on it: radiance is committed in iteration order. */
    int32_t max_batch;        /* largest `count` pt_iterate_batch will be given (sizes the path pools: two pools of
                                 44 B x pixels x max_batch per slot plus ~10 % of chunk slack -- 81 MB per iteration of a
                                 1280x720 frame and slot; 32 B and 59 MB where the scene takes the PLAIN kernels -- and pixels x max_batch must stay below 2^29);
                                 0 = 1, max PT_MAX_BATCH */
    void   *stream;           /* hipStream_t to enqueue on; NULL = the default stream */
    float  *accum_dev;        /* optional caller-owned device accumulator, W*H*3 floats (or the shard's rows only
                                 with PT_FLAG_ACCUM_SHARD_ROWS), zeroed by the caller (e.g. a torch tensor that
                                 RCCL exchanges); NULL = owned by the library like dev_image (pathtrace.cu:71,80-81) */
    /* README extras the reference names but does not implement; 0 = off = the reference's pinhole camera.
     * Depth of field by jittering rays within an aperture (README.md:100-101): camera rays start at a uniformly sampled
     * point of a lens disc of this radius around the eye and pass through the point their pinhole ray reaches at
     * focal_distance along the view axis.  (Imperfect specular, README.md:171-185, needs no option: a material with
     * REFL > 0 and SPECEX > 0 scatters into the Phong lobe of that exponent around the mirror direction.) */
    float   lens_radius;
    float   focal_distance;
} PtOptions;

#define PT_MAX_DEPTH 62
#define PT_MAX_BATCH 256

/* ---- motion blur (PT_FLAG_MOTION) ---------------------------------------------------------------------------------------------------
 * "Some method of defining object motion, and motion blur by averaging samples at different times" (the course README's extra): a frame
 * averages iterations, so an iteration that sees the scene at ONE time of the shutter is a sample at that time.
 *
 * Under the flag `geoms` of a full pt_init holds PT_MOTION_STEPS x ngeoms records: step s's scene is geoms[s * ngeoms .. (s + 1) * ngeoms),
 * the scene at shutter time t_s = (s + 0.5) / PT_MOTION_STEPS.  The library knows no time and interpolates nothing: the caller supplies each
 * step's complete PtGeom, matrices included.  Steps must agree on every geom's type and materialid; what pt_set_meshes, pt_set_textures and
 * pt_set_bump_maps registered applies to geom g of every step.
 *
 * Iteration i renders step PT_MOTION_STEP(i): runs of PT_MOTION_RUN consecutive iterations share a step (an aligned batch of 8 is one set
 * of launches), and the runs visit the steps in bit-reversed order, so that any prefix of a cycle of PT_MOTION_STEPS x PT_MOTION_RUN = 128
 * iterations spreads over the shutter.  The step is a function of i alone: batching never changes a frame.  pt_iterate_batch cuts its
 * range at run boundaries and does for each piece what it does for a whole call; PT_FLAG_TRACE_AHEAD's batches end with their run.
 *
 * THE LAW: after iterations 1..n both accumulators, PtCounters and every read-back equal, bit for bit, what comes of adding, in iteration
 * order, iteration i of an unflagged renderer initialised with step PT_MOTION_STEP(i)'s geoms.
 *
 * The renderer plans all 16 steps before anything is touched; a step that is refused refuses the call, and the message names the step.  The
 * steps may take different forms of k_bounce; what the in-flight slots share (pool sizes, path layout, batch size, frame) must agree across
 * steps, else PT_ERR_INVALID.  Texels and mesh records, which no pose changes, are held once.  Row shards, PT_FLAG_MOMENTS,
 * PT_FLAG_DIRECT_LIGHTING (emitters per step), PT_FLAG_MIXTURE_WEIGHTED, PT_FLAG_TRACE_AHEAD, a thin lens and PT_FLAG_KERNEL_TIMING go with
 * the flag.  On a flagged renderer pt_denoise*, pt_gbuffer are refused (a first-hit guide has no single pose), and the same-scene camera
 * move runs the full call inside with all 16 steps.
 *
 * Known costs: 16 poses are 16 ghosts when an object moves by much more than its own size on screen, and a frame of n iterations weights
 * the steps equally only when n is a multiple of 128. */
#define PT_MOTION_STEPS 16
#define PT_MOTION_RUN 8
/* bitrev4(((i - 1) / PT_MOTION_RUN) % PT_MOTION_STEPS), i >= 1 */
#define PT_MOTION_BITREV4(r) (((((r) >> 0) & 1) << 3) | ((((r) >> 1) & 1) << 2) | ((((r) >> 2) & 1) << 1) | (((r) >> 3) & 1))
#define PT_MOTION_STEP(i) PT_MOTION_BITREV4((((i) - 1) / PT_MOTION_RUN) % PT_MOTION_STEPS)
/* Bumped whenever a struct of this header changes size or meaning (7: PtTexture / PtTexBinding, pt_set_textures; 6: round 6 -- pt_group_iterate / pt_group_reduce, the group's asynchronous
 * assembly; 5: contexts and groups; PtMesh has carried `normals` and `materials` since 4).  A host built against another header finds out with
 * pt_abi_version() != PT_AMD_ABI_VERSION before it passes structs. */
#define PT_AMD_ABI_VERSION 7
int pt_abi_version(void);

typedef struct PtCounters {
    int64_t live[PT_MAX_DEPTH + 2]; /* live[d] = paths entering bounce d (d = 1..depth), summed over   */
    int64_t light_hits;             /*           every iteration since pt_init / pt_counters_reset      */
    int64_t misses;                 /* traced paths that hit nothing (diagnostic: paths of the last bounce that certainly
                                       cannot reach an emitter are not traced and appear in neither tally)          */
    int64_t iterations;
    int64_t bounce_launches;        /* bounce-kernel launches covered by bounce_kernel_ms               */
    double  bounce_kernel_ms;       /* sum of HIP-event durations (PT_FLAG_KERNEL_TIMING only)          */
    double  raygen_kernel_ms;
    int64_t raygen_launches;
    int64_t ended_early[PT_MAX_DEPTH + 2]; /* of live[d]: paths whose scatter at bounce d - 1 certainly misses every primitive (scenes
                                              whose primitives are all walls or binned): tallied as entering bounce d and missing,
                                              which is what they do, but never written to or read from the path pools */
} PtCounters;

/* Triangle meshes (README.md:112-116 "arbitrary mesh loading and rendering", README.md:236 object type "mesh"; the reference
 * names them and `glm::intersectRayTriangle` and holds no mesh code, so the semantics are build-defined -- oracle/pt_oracle.cpp,
 * mesh_intersection_test):
 *   - a PtGeom of type PT_MESH carries its transform like any primitive; its triangles are in OBJECT space (the OBJ file's
 *     coordinates), 9 floats each (v0, v1, v2), counter-clockwise = front ("outside");
 *   - the ray is taken to object space like the sphere test does (src/intersections.h:104-110); the triangle test is
 *     glm::intersectRayTriangle (glm/gtx/intersect.inl:36-72) made two-sided; a triangle is tested when the ray passes the
 *     slab test of the triangle's bounding box (inflated by 1e-5 of the mesh's largest |coordinate|; plane parameters
 *     fma(plane, 1/d, -(o * 1/d)), compared with a relative slack of 1e-5) and its hit counts at or
 *     beyond that box's entry -- true of every geometric hit, and what lets a bounding-volume hierarchy return exactly the
 *     brute-force result; nearest = smallest object-space t, ties to the lower triangle index; flat shading, the normal
 *     negated on the back side; hit point and distance as the sphere test's (getPointOnRay, transform, world distance).
 * pt_set_meshes registers the triangle soups of the scene's mesh geoms for the NEXT pt_init (copied; kept across pt_free, so the
 * reference's Free -> Init restart re-initialises the same scene; pt_set_meshes(NULL, 0) clears them).  pt_init fails with
 * PT_ERR_INVALID when a PT_MESH geom has no triangles or triangles are registered for a geom that is not a mesh. */
typedef struct PtMesh {
    int32_t geom;           /* index into pt_init's geoms */
    int32_t ntris;
    const float *tris;      /* ntris x 9 floats, finite */
    /* README.md:112-116 leftovers (round 4), both optional:
     *   normals    ntris x 9 floats: the vertex normals n0, n1, n2 of every triangle, object space (an OBJ's `vn`).  The shading normal
     *              of a hit is then the barycentric blend n0 (1 - u - v) + n1 u + n2 v with the hit's own (u, v), turned to the side the
     *              counter-clockwise face normal points to and normalised (a blend of length zero keeps the face normal); everything
     *              else -- which side is "outside", the hit point, the invTranspose map to world space -- as for flat shading.
     *              The blended normal is the one the hit is SHADED with: reflection and its SPECEX lobe, refraction and Schlick's cosine,
     *              the diffuse hemisphere, the direct-lighting cosine, the denoiser's guide normal -- and the new ray's origin, which sits
     *              0.001 along it (against it for a refracted ray) from the hit point.  Which side of the surface the ray came from, and
     *              with it eta, stays the geometric question.  The new origin lies on the geometric side its branch names as long as
     *              0.001 (Ns . N) exceeds the 0.0001 object-space step the hit point is taken short of the surface, seen along N
     *              (at most 0.0001 x the largest scale): normals bent by less than ~70 degrees on objects of scale <= 3.
     *   materials  ntris scene materials, one per face (an OBJ's `usemtl <k>`); -1 = the object's own.  The FACE's material is the one
     *              that scatters the path, ends it (an emissive face, which adds (colour x its RGB) x its emittance) or lets it go on
     *              (a face without emittance on an emissive object).
     *              pt_init fails with PT_ERR_INVALID on an id >= nmats. */
    const float *normals;   /* or NULL: flat shading */
    const int32_t *materials;   /* or NULL: every face takes the object's material */
} PtMesh;
int pt_set_meshes(const PtMesh *meshes, int nmeshes);
/* ... the same with the caller's sizeof(PtMesh): PT_ERR_INVALID instead of strided garbage when host and library disagree about the struct */
int pt_set_meshes_sized(const PtMesh *meshes, int nmeshes, size_t mesh_struct_bytes);

/* Texture mapping (PBRT 10.4; a README extra the reference names and does not implement, so the semantics are build-defined --
 * csrc/pt_device.h, "texture mapping", gives every operation):
 *   - a texture is bound to a PRIMITIVE (PtMaterial stays the reference's Material) and multiplies its material's colour (RGB) wherever the
 *     renderer uses it: the diffuse albedo and the emitted radiance.  SPECRGB and the material's switches are untouched; no random number is
 *     drawn and no path changes its course;
 *   - texels are linear float RGB, row 0 = the image's top row; repeat wrapping, bilinear filtering, v = 0 at the bottom (the OBJ convention);
 *   - texture coordinates: a mesh blends its triangles' corner UVs with the hit's barycentrics; a cube maps each face's square to [0, 1]^2
 *     (axis a: u = q[(a + 1) % 3] + 0.5, v = q[(a + 2) % 3] + 0.5 of the object-space hit point q); a sphere takes longitude and latitude
 *     of its object-space hit direction (u = 0.5 + atan2(z, x) / 2 pi, v = 0.5 + asin(y) / pi).
 * pt_set_textures registers textures and bindings for the NEXT pt_init (copied; kept across pt_free like pt_set_meshes' triangles;
 * (NULL, 0, ..., NULL, 0, ...) clears them); the struct sizes are the caller's sizeof, as pt_set_meshes_sized takes it.  pt_init fails with
 * PT_ERR_INVALID when a binding names a geom or texture out of range or a geom twice, a mesh binding has no UVs or another triangle count than
 * the registered mesh, a binding of a sphere or cube has UVs, a texel is non-finite, a side is outside 1..16384, or the textures hold 2^28 texels
 * or more.  Scenes with a bound texture take k_bounce instantiations of their own; other scenes run what they ran before. */
typedef struct PtTexture {
    int32_t width, height;
    const float *rgb;       /* width x height x 3 floats, row 0 = top */
} PtTexture;
typedef struct PtTexBinding {
    int32_t geom;           /* index into pt_init's geoms */
    int32_t texture;        /* index into the registered textures */
    int32_t ntris;          /* mesh geoms: the mesh's triangle count; spheres and cubes: 0 */
    const float *uvs;       /* mesh geoms: ntris x 6 floats, the corner UVs (u0, v0, u1, v1, u2, v2) of every triangle; others NULL */
} PtTexBinding;
int pt_set_textures(const PtTexture *textures, int ntextures, size_t texture_struct_bytes, const PtTexBinding *bindings, int nbindings,
                    size_t binding_struct_bytes);

/* Bump mapping (PBRT 10.5.1; a README extra the reference names and does not implement, so the semantics are build-defined --
 * csrc/pt_device.h, "bump mapping", gives every operation):
 *   - a height map -- one of the textures registered with pt_set_textures, channel 0, sampled as textures are -- and a scale (world units of
 *     displacement per unit of texel value) bound to a PRIMITIVE tilt the normal it is shaded with, by the height's central differences one
 *     texel apart along the texture coordinates textures use.  A height map needs no colour binding;
 *   - the tilted normal replaces the surface normal in refraction, mirror reflection, the SPECEX lobe, the diffuse hemisphere and the
 *     direct-lighting cosine; the ray's origin offset, the side (eta), emission and the texture colour keep the unbumped surface.  A path whose
 *     new direction would cross the geometric surface from its origin offset ends there, adding nothing.
 * pt_set_bump_maps registers bindings for the NEXT pt_init (copied; kept across pt_free; (NULL, 0, ...) clears them).  pt_init fails with
 * PT_ERR_INVALID when a binding names a geom or texture out of range or a geom twice, a mesh binding has no UVs or another triangle count than
 * the registered mesh, a binding of a sphere or cube has UVs, or a scale is non-finite.  Scenes with a bound height map take k_bounce
 * instantiations of their own; other scenes, textured ones included, run what they ran before.  (Additive: the ABI version stays.) */
typedef struct PtBumpBinding {
    int32_t geom;           /* index into pt_init's geoms */
    int32_t texture;        /* index into the textures registered with pt_set_textures */
    float scale;            /* finite */
    int32_t ntris;          /* mesh geoms: the mesh's triangle count; spheres and cubes: 0 */
    const float *uvs;       /* mesh geoms: ntris x 6 floats, the corner UVs (u0, v0, u1, v1, u2, v2) of every triangle; others NULL */
} PtBumpBinding;
int pt_set_bump_maps(const PtBumpBinding *bindings, int nbindings, size_t binding_struct_bytes);

/* pathtraceInit: upload scene, allocate the accumulator and the SoA path-state buffers.
 * Replaces reference src/pathtrace.cu:75-85.  Calling it twice without pt_free re-initialises (and, between two PT_FLAG_TEMPORAL renderers
 * of one resolution, is what carries the old view's samples over as the context's history: section "temporal reprojection").
 * A scene or an option that is refused -- every PT_ERR_INVALID -- is refused before anything is touched: nothing is allocated or released,
 * and the renderer that was there stays initialised and usable.  PT_ERR_NO_GPU and PT_ERR_HIP (a failed HIP call; pools that do not fit
 * the free device memory, which is measured after the old renderer has given its own back) leave the context without a renderer. */
int pt_init(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats,
            int traceDepth, const PtOptions *opts /* may be NULL */);

/* THE CAMERA MOVE: pt_init's same-scene form.  Called as
 *     pt_init(cam, NULL, 0, NULL, 0, PT_SAME_SCENE, NULL)
 * -- no geoms, no materials, PT_SAME_SCENE for the depth, no options: a call that was refused before -- it moves the camera of the live
 * renderer in place.  The observable result is that of
 *     pt_init(cam, <the geoms, materials, traceDepth and options the live renderer was initialised with>)
 * called over the live renderer: the library's accumulators, second moments and albedo sums are zeroed (a caller-owned accum_dev stays
 * the caller's to zero), the counters and the committed count start again, batches traced ahead are discarded, guide buffers are
 * invalidated, and under PT_FLAG_TEMPORAL the old view is captured into the context's history first, exactly as the full call captures it
 * (PT_FLAG_DEMOD_HISTORY's albedo included; an old view without a committed iteration leaves the history as it was).  The meshes, textures
 * and height maps are the ones the renderer was initialised with, not those registered since.  Everything rendered, read back, filtered or
 * displayed afterwards is bit for bit what it would be after the full call.
 * What it saves is the cost: the renderer keeps its copy of the scene arguments, so where the new plan needs the allocations the renderer
 * holds -- the same kernels and sizes; no planned size depends on the camera -- every device buffer, stream, event and pinned registration
 * is kept, the work list's per-pixel face certificates are evaluated on the device, and only the tables whose bytes differ are uploaded
 * (textures and mesh records never).  Otherwise, and for a renderer that carries a sticky device fault, it runs the full call inside.
 * PT_ERR_NOT_INIT without a renderer; PT_ERR_INVALID for a NULL camera, a resolution other than the live renderer's, or a camera the full
 * call would refuse -- each before anything is touched: the renderer stays usable with its old view.  A HIP call that fails before
 * anything has been overwritten makes it run the full call instead; one that fails later leaves the context without a renderer, as the
 * full call's do.  Acts on the calling thread's current context.  (Additive, and no new function: the ABI version stays.) */
#define PT_SAME_SCENE 0

/* pathtrace(pbo, frame, iter): one iteration (1 spp), iter is 1-based like src/main.cpp:97-103.
 * Enqueues camera-ray generation, traceDepth fused intersect+shade+compact launches and, when
 * rgba8_dev != NULL, the sendImageToPBO conversion (src/pathtrace.cu:48-68) into that DEVICE
 * buffer of W*H uchar4 -- under PT_FLAG_DISPLAY_FILTER the variance-guided filter's bytes instead of the raw accumulator's (section
 * "display filter" below).  Asynchronous on the configured stream.  Replaces src/pathtrace.cu:123-167. */
int pt_iterate(int frame, int iter, void *rgba8_dev /* may be NULL (headless) */);

/* `count` consecutive iterations first_iter .. first_iter+count-1 traced as ONE wavefront (their paths share the
 * bounce launches, which makes each launch `count` times larger: fewer, fatter launches for small frames or
 * small multi-GPU shards).  The result is identical to `count` pt_iterate calls: every pixel still receives its
 * samples in iteration order.  rgba8_dev, if given, is converted with iter = first_iter+count-1.
 * pt_iterate(frame, iter, pbo) == pt_iterate_batch(frame, iter, 1, pbo). */
int pt_iterate_batch(int frame, int first_iter, int count, void *rgba8_dev);

/* Wait for every stream the renderer uses; reports device-side faults (PT_ERR_DEVICE).  (checkCUDAError's sync,
 * pathtrace.cu:23.)  Without a renderer it waits for the scan library's work on every stream. */
int pt_sync(void);

/* Copy the un-normalised running sum (W*H*3 floats, index = x + y*W) to host: the D2H copy of
 * src/pathtrace.cu:170-171 into scene->state.image.  Synchronises. */
int pt_readback(float *rgb_sum_host);

/* Page-lock a caller-owned host buffer (e.g. scene->state.image) so that pt_readback into it runs at PCIe rate instead of
 * through the runtime's pageable staging copy: the per-iteration D2H copy of the reference protocol (pathtrace.cu:170-171).
 * The caller keeps the memory alive until pt_unpin_host / pt_free, which release the registration; one buffer at a time.
 * Purely an optimisation: pt_readback works with any host pointer. */
int pt_pin_host(void *host, size_t bytes);
int pt_unpin_host(void);

/* sendImageToPBO into a HOST buffer (W*H*4 bytes). Synchronises.  (Under PT_FLAG_DISPLAY_FILTER: the display filter's bytes, as pt_iterate's.) */
int pt_readback_rgba8(int iter, uint8_t *rgba_host);

/* ---- denoiser: an edge-avoiding a-trous wavelet filter over the image, guided by first-hit position and normal (Dammertz et al., HPG 2010;
 * csrc/pt_denoise.h gives every operation, tests/denoise_ref.py restates it).  `levels` passes of a 5 x 5 B3-spline stencil whose taps lie
 * 2^level pixels apart; a tap's weight falls with the squared differences of colour (sigma_color, halved per level), guide normal (sigma_normal)
 * and guide position (sigma_position, world units): w = h * exp(-(|dc|^2 / sc^2 + |dn|^2 / sn^2 + |dp|^2 / sp^2)); a sigma of +inf switches its
 * term off (all three: the plain blur).  A pixel that hit something and one that hit nothing never mix.
 * The guide buffers are the nearest hits of the camera rays iteration `guide_iter` traces (its jitter, and its lens sample with depth of field):
 * world-space point and distance, the un-bumped shading normal, the primitive's index (-1, distance -1 and zeros for a miss).
 *   pt_denoise         filters the accumulator's mean over `samples` (sum / samples) into rgb_mean_host, W*H*3 floats
 *   pt_denoise_rgba8   ... and applies sendImageToPBO's conversion to it: clamp((int)(mean * 255.0), 0, 255), W*H*4 bytes
 *   pt_gbuffer         the guide buffers themselves
 * All three run on the context's stream behind every iteration committed so far, synchronise like pt_readback and leave the accumulator
 * untouched (a caller-owned accum_dev too): rendering may go on afterwards.  Guide and filter buffers are allocated on first use and freed by
 * pt_free / pt_init; the guide buffers are kept for the guide_iter they were made for until then.
 * PT_ERR_NOT_INIT before pt_init; PT_ERR_INVALID for levels outside 1..8, a sigma that is 0, negative or NaN, guide_iter < 1, samples < 1,
 * another struct size than this header's, and for a renderer initialised with shard_count > 1 or PT_FLAG_ACCUM_SHARD_ROWS (its accumulator
 * is not a frame).  Device groups are out of scope: pt_group_* has no denoiser; filter what pt_group_readback returns in a context of its own.
 * (Additive: the ABI version stays.) */
typedef struct PtDenoiseParams {
    int32_t levels;          /* 1..8 */
    int32_t guide_iter;      /* >= 1: the iteration whose camera rays give the guide buffers */
    float sigma_color, sigma_normal, sigma_position;   /* > 0, +inf allowed; NaN, 0, negatives refused */
} PtDenoiseParams;
int pt_denoise(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, float *rgb_mean_host /* W*H*3 */);
int pt_denoise_rgba8(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, uint8_t *rgba_host);
int pt_gbuffer(int guide_iter, float *pos_t_host /* W*H*4 */, float *nrm_host /* W*H*3 */, int32_t *geom_host /* W*H */);

/* ---- per-pixel variance and the variance-guided filter (a renderer initialised with PT_FLAG_MOMENTS; csrc/pt_denoise.h gives every operation,
 * tests/denoise_var_ref.py restates it).  S = the accumulator's RGB sum, Q = the sum of the samples' squared luminance, n = samples:
 *   pt_readback_moments   Q, W*H floats
 *   pt_variance           the variance of every pixel's MEAN luminance: c = S / n, L = lum(c), d = max(Q / n - L * L, 0), v = d / (n - 1)
 *   pt_denoise_var        the a-trous filter of pt_denoise with SVGF's colour term (Schied et al., HPG 2017) in place of sigma_color: a tap's weight
 *                         falls with (lum(c_q) - lum(c_p))^2 / (sigma_lum^2 * g + 1e-8), g the 3 x 3 Gaussian-filtered variance around p, so ONE
 *                         sigma_lum serves every sample count: noisy pixels blur, converged detail stays.  The variance is filtered along with
 *                         the colour (weights squared) and passed from level to level; var_host (or NULL) receives the last level's.
 *   pt_denoise_var_rgba8  ... and sendImageToPBO's conversion of the filtered mean, as pt_denoise_rgba8
 * Guides, stencil, sigma_normal / sigma_position, guide_iter, the stream, the synchronisation and the buffers' lifetime are pt_denoise's; both
 * accumulators are left untouched.  PT_ERR_NOT_INIT before pt_init; PT_ERR_INVALID without PT_FLAG_MOMENTS, for samples < 2, levels outside
 * 1..8, a sigma that is 0, negative or NaN (+inf switches its term off), guide_iter < 1 and another struct size than this header's.
 * (Additive: the ABI version stays.) */
int pt_readback_moments(float *lum_sq_sum_host /* W*H */);
int pt_variance(int samples, float *var_mean_host /* W*H */);
typedef struct PtDenoiseVarParams {
    int32_t levels;          /* 1..8 */
    int32_t guide_iter;      /* >= 1 */
    float sigma_lum, sigma_normal, sigma_position;   /* > 0, +inf allowed; NaN, 0, negatives refused */
} PtDenoiseVarParams;
int pt_denoise_var(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, float *rgb_mean_host /* W*H*3 */,
                   float *var_host /* W*H or NULL */);
int pt_denoise_var_rgba8(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, uint8_t *rgba_host);

/* ---- render to a noise threshold (a renderer initialised with PT_FLAG_MOMENTS; csrc/pt_noise.h gives every operation, tests/noise_ref.py
 * restates it).  The frame is judged per tile of PT_NOISE_TILE x PT_NOISE_TILE pixels, not per pixel: a pixel whose samples all missed the
 * light has variance 0 and looks converged, while a tile's summed variance is an unbiased estimate.  With v, L of pt_variance per pixel:
 *   r(tile) = (sum v / N) / max(sum L / N, lum_floor)^2,  N = the tile's pixels inside the frame;  sqrt(r) = the tile's relative standard error
 *   a tile is unconverged iff r > threshold * threshold (fp32; a NaN r is not);  max_rel_var = the largest r of the frame, NaN ignored
 *   pt_noise_stats     the statistics of the accumulator as `samples` iterations left it; tile_rel_var_host (or NULL) receives r[ty][tx].  Runs
 *                      on the context's stream behind every commit and synchronises, like pt_variance; both accumulators are left untouched.
 *                      out->converged is judged with a fraction of 0: no tile above the threshold.
 *   pt_iterate_until   renders iterations first_iter, first_iter + 1, ... (the accumulator holds 1 .. first_iter - 1) in rounds of check_every
 *                      -- the last one cut at max_samples; each round pt_iterate_batch calls of at most max_batch -- and after every round that
 *                      ends with at least min_samples checks the frame on the device: it is converged when
 *                      unconverged <= floor((double)max_unconverged_fraction * tiles).  lookahead 0: the host waits for each check before it
 *                      enqueues more; *samples_done = s*, the first checked count that is converged.  lookahead 1: the next round is enqueued
 *                      BEFORE the host waits for the check (for the check's event alone), so the GPU never idles for the decision and that
 *                      round counts: *samples_done = min(s* + check_every, max_samples).  Never converged: max_samples.  Deterministic either
 *                      way, and both accumulators equal pt_iterate_batch over iterations 1 .. *samples_done bit for bit.  `out`: the
 *                      statistics of the final accumulator, with out->converged = how the loop ended.  Returns PT_OK either way; synchronises
 *                      and reports a device fault as pt_sync does.  samples_done may be NULL.
 * PT_ERR_NOT_INIT before pt_init; PT_ERR_INVALID without PT_FLAG_MOMENTS (row shards and device groups refuse that flag), with
 * PT_FLAG_TRACE_AHEAD in effect (pt_iterate_until), for samples < 2, min_samples < 2, max_samples < 2, a threshold or lum_floor that is not
 * finite and > 0, a fraction outside 0..1 or NaN, check_every < 1, first_iter < 1, max_samples < first_iter or beyond the last iteration,
 * lookahead other than 0 or 1, a null `out` or target and another struct size than this header's.  (Additive: the ABI version stays.) */
#define PT_NOISE_TILE 16
typedef struct PtNoiseStats {
    int32_t samples, tiles_x, tiles_y, converged;
    int64_t tiles, unconverged;
    float max_rel_var, thr2;     /* thr2 = threshold * threshold, what the tiles' r was compared with */
} PtNoiseStats;
int pt_noise_stats(int samples, float threshold, float lum_floor, PtNoiseStats *out, size_t stats_struct_bytes,
                   float *tile_rel_var_host /* tiles_y * tiles_x, or NULL */);
typedef struct PtNoiseTarget {
    float threshold, lum_floor, max_unconverged_fraction;
    int32_t min_samples, max_samples, check_every, lookahead;
} PtNoiseTarget;
int pt_iterate_until(int frame, int first_iter, const PtNoiseTarget *t, size_t target_struct_bytes, PtNoiseStats *out, int32_t *samples_done);

/* ---- temporal reprojection (PT_FLAG_TEMPORAL; the temporal half of SVGF, Schied et al., HPG 2017, for a static scene under a moving pinhole
 * camera; csrc/pt_temporal.h gives every operation, tests/temporal_ref.py restates it).  No function of its own: a flag, and what pt_init,
 * pt_free and pt_denoise_var do under it.
 *   HISTORY belongs to the context: per pixel of the OLD view its mean colour, mean squared luminance and effective sample count (at most
 *   PT_TEMPORAL_MAX_HISTORY), that view's guide buffers of guide_iter 1 and its camera.  It is made at one moment only: pt_init called over a
 *   live renderer (the "calling it twice re-initialises" path), or its same-scene form (PT_SAME_SCENE), which is that call with the renderer's own scene, when the old and the new renderer both carry the flag and have the same
 *   resolution, the new scene has been accepted, and the old renderer has committed at least one iteration (its sample count is the number of
 *   iterations it committed since its pt_init -- pt_counters_reset, which leaves the accumulators alone, leaves that count alone too).  The capture is recursive: what is kept is the old view's own blend of ITS history with ITS samples, so a camera
 *   dragged through many views of a few samples each keeps accumulating up to the cap.  An old renderer without a committed iteration leaves
 *   the history there was, with the camera it was made for.  An old view whose guide buffers cannot be made (pt_gbuffer's PT_ERR_INVALID: a
 *   mesh hierarchy too deep for its stacks) ends the history instead: pt_init drops it and goes on.  A HIP call that fails during the capture is
 *   PT_ERR_HIP like any other of pt_init's, and leaves the context without a renderer.  pt_free, pt_ctx_destroy, the exit handler and a pt_init without the flag or with
 *   another resolution drop it; a refused pt_init leaves it as it was.  "The same scene" is the caller's promise: a caller that changes the scene
 *   calls pt_free first.
 *   pt_denoise_var / pt_denoise_var_rgba8 of a renderer whose context holds history: the new pixel's first hit (the guide buffers of the call's
 *   guide_iter) is projected into the old camera; of the four old pixels around it those count that hold history, show the same primitive, a
 *   normal within dot >= PT_TEMPORAL_NORMAL_DOT and lie within PT_TEMPORAL_PLANE_FRACTION * t of the new hit's tangent plane (t: the new hit's
 *   distance); their bilinear weights must add up to more than PT_TEMPORAL_MIN_WEIGHT.  History hc of count Nh and the new sums S, Q of n
 *   samples blend to c = (hc Nh + S) / (Nh + n), m2 = (hm2 Nh + Q) / (Nh + n), variance max(m2 - lum(c)^2, 0) / (Nh + n - 1): level 0 of the
 *   filter reads that image instead of the accumulators' mean and variance.  A pixel without valid history (a disocclusion, the frame's edge)
 *   gets exactly what it got without the flag. */
#define PT_TEMPORAL_MAX_HISTORY 32.0f
#define PT_TEMPORAL_NORMAL_DOT 0.9f
#define PT_TEMPORAL_PLANE_FRACTION 0.01f
#define PT_TEMPORAL_MIN_WEIGHT 0.5f

/* ---- display filter (PT_FLAG_DISPLAY_FILTER, with PT_FLAG_MOMENTS): the variance-guided filter where the display reads it.  No function of its
 * own: a flag, and what the calls that write sendImageToPBO's bytes of the accumulator do under it.
 *   pt_iterate / pt_iterate_batch with rgba8_dev != NULL write into rgba8_dev, and pt_readback_rgba8 returns, the bytes
 *   pt_denoise_var_rgba8(n, &{PT_DISPLAY_LEVELS, PT_DISPLAY_GUIDE_ITER, PT_DISPLAY_SIGMA_LUM, PT_DISPLAY_SIGMA_NORMAL, PT_DISPLAY_SIGMA_POSITION},
 *   ...) would return at that point of the stream: n is the count those calls divide by today (first_iter + count - 1, resp. iter), and where
 *   the context holds history (PT_FLAG_TEMPORAL) the bytes include the blend with it.  With n == 1 -- a variance needs two samples -- the bytes
 *   are the unfiltered conversion, as without the flag (unless PT_FLAG_SPATIAL_VARIANCE estimates one: section "spatial variance" below).
 *   pt_iterate_batch enqueues the filter on the renderer's stream behind the commit: the guide buffers (once per renderer, while no pt_denoise*
 *   or pt_gbuffer call asks for another guide_iter), the blend with the history where there is one, the levels, the last of which writes the
 *   bytes itself.  No host synchronisation, no allocation: pt_init allocates the filter's buffers (guide buffers, two float4 images, one image of
 *   bytes: 68 bytes per pixel) and counts them in its memory check.  pt_denoise_var* calls with other parameters share those buffers on the
 *   same stream; each call's result is its own.
 *   Both accumulators, pt_readback, pt_readback_moments, pt_variance, pt_noise_stats, pt_iterate_until, pt_denoise*, pt_gbuffer and the capture of
 *   history are the unflagged renderer's bit for bit.
 *   pt_init answers PT_ERR_INVALID, before anything is touched, to the flag without PT_FLAG_MOMENTS (so: with row shards, and from
 *   pt_group_init) and for a scene whose guide buffers cannot be made (pt_gbuffer's PT_ERR_INVALID: a mesh hierarchy too deep for its stacks).
 *   PT_FLAG_TRACE_AHEAD, a thin lens and direct lighting go with it.
 * The setting -- the calls have no room for parameters -- is pt_denoise_var's default, the one that serves every sample count: */
#define PT_DISPLAY_LEVELS 5
#define PT_DISPLAY_GUIDE_ITER 1
#define PT_DISPLAY_SIGMA_LUM 4.0f
#define PT_DISPLAY_SIGMA_NORMAL 0.35f
#define PT_DISPLAY_SIGMA_POSITION 2.0f

/* ---- spatial variance (PT_FLAG_SPATIAL_VARIANCE, with PT_FLAG_MOMENTS; SVGF's estimate for pixels of short history, Schied et al., HPG 2017,
 * section 4.2; csrc/pt_spatial_var.h gives every operation, tests/spatial_var_ref.py restates it).  No function of its own: a flag, and what
 * pt_denoise_var*, and under PT_FLAG_DISPLAY_FILTER the display path, do under it.
 *   One sample has no variance, so without the flag pt_denoise_var* refuse samples < 2, the display's first frame is the raw conversion, and
 *   under PT_FLAG_TEMPORAL a disoccluded pixel of a one-sample view stays a raw sample inside a filtered frame.  Under the flag
 *   pt_denoise_var / pt_denoise_var_rgba8 accept samples >= 1.  With samples == 1 two launches go in front of the filter's levels: the
 *   pixel's mean colour, mean squared luminance m2 and effective sample count N (with history under PT_FLAG_TEMPORAL: the blend's, N = Nh + n
 *   uncapped; without: S / n, Q / n, n), and then per pixel the variance level 0 reads:
 *     N >= PT_SPATIAL_MIN_COUNT   the pixel's own, max(m2 - lum(c)^2, 0) / (N - 1): what it gets without the flag, to the bit
 *     otherwise                   over the (2 PT_SPATIAL_RADIUS + 1)^2 window around it, weighted by the filter's normal and position terms
 *                                 (the call's sigma_normal, sigma_position; the centre 1; never across the hit / miss border):
 *                                 M1 = sum w lum(c_q) / sum w, M2 = sum w m2_q / sum w, variance max(M2 - M1^2, 0) / N -- N, not N - 1: the
 *                                 mean comes from the window, not from the pixel
 *   With samples >= 2 no pixel's count is below 2 and the renderer enqueues exactly the launches it enqueues without the flag.
 *   With PT_FLAG_DISPLAY_FILTER the display path filters at n == 1 too: pt_iterate(.., rgba8_dev) and pt_readback_rgba8 give the bytes
 *   pt_denoise_var_rgba8(1, PT_DISPLAY_*) would return.  No host synchronisation, no allocation: pt_init allocates the one image the flag adds
 *   (W*H floats, the counts) and counts it in its memory check.
 *   pt_variance, pt_noise_stats and pt_iterate_until keep their samples >= 2; both accumulators and everything else are the unflagged
 *   renderer's bit for bit.  pt_init answers PT_ERR_INVALID, before anything is touched, to the flag without PT_FLAG_MOMENTS (so: with row
 *   shards, and from pt_group_init).  PT_FLAG_TEMPORAL, PT_FLAG_DISPLAY_FILTER, PT_FLAG_TRACE_AHEAD, direct lighting and a thin lens go with it.
 * PT_SPATIAL_RADIUS is chosen by the study of tests/test_spatial_var_cpu.py (README, "Spatial variance"). */
#define PT_SPATIAL_MIN_COUNT 2.0f
#define PT_SPATIAL_RADIUS 1

/* ---- demodulation (PT_FLAG_DEMODULATE, with PT_FLAG_MOMENTS; csrc/pt_albedo.h gives every operation, tests/demod_ref.py restates it).  No
 * function of its own: a flag, and what pt_iterate*, pt_denoise_var* and, under PT_FLAG_DISPLAY_FILTER, the display path do under it.
 *   The variance-guided filter handles textures worst: a texel border under its stencil is an edge the luminance term can only keep by
 *   keeping the noise.  Under the flag the filter's levels see the light that reaches the surface instead: every pixel's colour is divided by
 *   its MEAN first-hit albedo A over the very iterations that were committed, filtered, and multiplied by A again.
 *   The albedo accumulator: pt_init allocates one more image of its own, W*H float4 (.xyz the albedo sum, .w the number of iterations added),
 *   zeroed, and counts it in its memory check.  Every pt_iterate / pt_iterate_batch -- pt_iterate_until's rounds included -- enqueues one
 *   more launch for its iterations first_iter .. first_iter + count - 1 on the renderer's stream, without a host synchronisation: per pixel
 *   and iteration the nearest hit of the camera ray the renderer traces (its jitter, its lens sample), found as pt_gbuffer finds it, adds
 *     (1, 1, 1)                                  for a miss, and for a hit whose material emits, reflects or refracts (emittance > 0,
 *                                                hasReflective > 0, hasRefractive > 0; a mesh face's own material where it has one)
 *     material colour x the bound texture's texel  otherwise: the colour the path is multiplied with at that hit, to the bit
 *   in ascending order of the iterations, one fp32 addition per channel: a batch equals its single calls bit for bit.
 *   The filter: with n = (float)samples and eps = PT_DEMOD_MIN_ALBEDO, A.k = max(Asum.k / n, eps) (a NaN gives eps).  In front of level 0 the
 *   pixel's (c, v) -- the accumulators' mean and variance, or at one sample under PT_FLAG_SPATIAL_VARIANCE the estimate's -- becomes
 *   (c / A, v rho^2), rho = lum(c / A) / lum(c) (1 where lum(c) is not positive): the relative standard error of the luminance is kept.  The
 *   levels run as without the flag, level 0 as a later level at step 1.  The last level stores co * A for its filtered colour co and, where
 *   the variance is asked for, vo rho'^2 with rho' = lum(co * A) / lum(co) (1 where lum(co) is not positive) -- or the bytes of co * A, so
 *   the display path stays one fused launch.
 *   pt_denoise_var, pt_denoise_var_rgba8 and, with PT_FLAG_DISPLAY_FILTER, pt_iterate(.., rgba8_dev) / pt_readback_rgba8 give that result;
 *   their `samples` refusals stay.  `samples` should be the number of iterations committed: the sums are divided by it.
 *   Both accumulators, every other read-back, pt_variance, pt_noise_stats, pt_iterate_until, pt_denoise and pt_gbuffer are the unflagged
 *   renderer's bit for bit, and a renderer without the flag launches exactly what it launched before.
 *   pt_init answers PT_ERR_INVALID, before anything is touched, to the flag without PT_FLAG_MOMENTS (so: with row shards, and from
 *   pt_group_init), with PT_FLAG_TEMPORAL (history carries no albedo yet -- unless PT_FLAG_DEMOD_HISTORY is given: "demodulated history" below), with PT_FLAG_TRACE_AHEAD (judged on the caller's flags), and for a
 *   scene whose guide buffers cannot be made.  A thin lens, direct lighting, PT_FLAG_DISPLAY_FILTER and PT_FLAG_SPATIAL_VARIANCE go with it.
 *   Known cost: mirrors, glass and lights stay un-demodulated; at high sample counts on textures with (nearly) black texels the floor eps
 *   makes the demodulated filter lose a little to the plain one (README, "Demodulation").
 * PT_DEMOD_MIN_ALBEDO is chosen by the study of tests/test_demod_cpu.py among 1/256, 1/64 and 1/16 (README, "Demodulation"). */
#define PT_DEMOD_MIN_ALBEDO 0.015625f

/* ---- demodulated history (PT_FLAG_DEMOD_HISTORY, with PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL | PT_FLAG_DEMODULATE; csrc/pt_temporal.h gives every
 * operation under "ALBEDO", tests/temporal_demod_ref.py restates it).  No function of its own: a flag.
 *   Without it a moving camera over a textured scene has to choose between history (PT_FLAG_TEMPORAL, which blurs texel borders through the
 *   luminance term) and demodulation (PT_FLAG_DEMODULATE, which starts again from one or two samples after every move, where one sample's
 *   albedo is a point sample of the texture).  SVGF accumulates demodulated light over time for this reason.
 *   History gains an image: pt_init over a live renderer that carries the flag also captures Ha' = (Ab, tot), the blend of ITS reprojected
 *   albedo history with ITS albedo sums (below), one more W*H float4 pair owned by the context.  History passes a pt_init only between two
 *   renderers that AGREE on the flag; where they differ it is dropped, as it is when the frame size changes.
 *   The blend: k_temporal's taps that count also add Ha[q] * w; ha = sumA / sumW (0 without history), and with Asum the renderer's albedo
 *   sums  Ab.k = (ha.k * Nh + Asum.k) / tot,  tot = Nh + n.  Without history that is Asum / n: PT_FLAG_DEMODULATE's mean albedo to the bit.
 *   The filter while the context holds history: the blend (c, v) of PT_FLAG_TEMPORAL -- at one sample under PT_FLAG_SPATIAL_VARIANCE the
 *   estimate's -- is divided by A = max(Ab, PT_DEMOD_MIN_ALBEDO) as PT_FLAG_DEMODULATE divides by its own, the levels run, and the last
 *   level multiplies back: Ab below PT_DEMOD_HISTORY_MIN_OWN samples (the reprojected albedo is anti-aliased but bilinearly blurred), the
 *   renderer's own mean albedo Asum / n from there on (sharp, but aliased at low counts).  pt_init allocates one more W*H float4 of its own
 *   for Ab and counts it in its memory check; the display path stays one fused last launch without a synchronisation or an allocation.
 *   Known cost: README, "Demodulated history".
 * PT_DEMOD_HISTORY_MIN_OWN is chosen by the study of tests/test_demod_history_cpu.py among 1, 2, 4, 8 and never (README, "Demodulated
 * history"). */
#define PT_DEMOD_HISTORY_MIN_OWN 2

/* ---- object history (PT_FLAG_OBJECT_HISTORY, with PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL; SVGF's reprojection through per-object motion;
 * csrc/pt_temporal.h gives every operation under "MOTION", tests/temporal_motion_ref.py restates it).  No function of its own: a flag, and
 * what pt_init does under it.
 *   Without it history survives a camera move and nothing else: "the same scene" is the caller's promise, and a caller that nudges a sphere
 *   either calls pt_free -- every pixel starts again, the nine tenths of the frame that did not change included -- or breaks the promise.
 *   When history passes: between two renderers that BOTH carry the flag (where they differ it is dropped, as under PT_FLAG_DEMOD_HISTORY),
 *   next to PT_FLAG_TEMPORAL's conditions, pt_init compares the call with what the live renderer was initialised with: ngeoms; every geom's
 *   type and materialid; nmats and the materials' bytes; and what is registered NOW with pt_set_meshes / pt_set_textures / pt_set_bump_maps
 *   against the renderer's own copies, byte for byte (PT_FLAG_KEEP_RENDERER's comparison: memcmp, no hash).  translation, rotation, scale
 *   and the three matrices may differ.  Any other difference drops the history and the call goes on as a full call without one.  A refused
 *   pt_init leaves everything as it was.
 *   The motion table: for every primitive g the host forms A = T_old[g] Tinv_new[g] in double -- `transform` of the geoms the history's
 *   view was rendered with, `inverseTransform` of the call's: the new world to the old -- and rounds rows 0..2 once to fp32, m[3][4]; and
 *   the inverse transpose of A's linear part, by cofactors over the determinant in double, rounded once, G[3][3].  A primitive whose
 *   transform and inverseTransform are byte-equal on both sides is UNMOVED (state 0), one with a non-finite number among the 21 has NO
 *   HISTORY (state 2: a zero scale), every other MOVED (state 1).  The table belongs to the context's history, beside the old camera.  With
 *   every primitive unmoved -- always so for the same-scene form and for a repeated identical call -- the history holds no table and the
 *   renderer launches exactly the kernels of PT_FLAG_TEMPORAL.  Chains work as the camera's do: the capture at the next pt_init reprojects
 *   with the table the going renderer got at ITS pt_init; only then is the table for the coming view made.
 *   The reprojection of a moved primitive's pixel: its hit P and normal N go to the old world first, P' = m (P, 1), N' = G N / |G N| (no
 *   history where that length is not positive), and PT_FLAG_TEMPORAL's projection and tap tests take P' and N'; the plane test's distance
 *   stays the new hit's own.  An unmoved primitive's pixel takes PT_FLAG_TEMPORAL's bits.
 *   The cap: light changes when an object moves -- its shadow, its bounce light -- while the unmoved background passes every test and keeps
 *   the old light.  A view whose table holds a moved primitive therefore blends with the history's count capped at PT_OBJECT_HISTORY_MAX in
 *   the place of PT_TEMPORAL_MAX_HISTORY, so that the new samples wash the stale light out faster.  Stale light is not detected otherwise.
 *   PT_FLAG_DEMOD_HISTORY, PT_FLAG_DISPLAY_FILTER (which still allocates nothing and waits for nothing: pt_init uploads the table),
 *   PT_FLAG_SPATIAL_VARIANCE, PT_FLAG_KEEP_RENDERER, direct lighting and the same-scene form go with it.  Out of scope: deforming meshes,
 *   objects added or removed and material edits (each drops the history), a thin lens, groups and row shards.
 * PT_OBJECT_HISTORY_MAX is chosen by the study of tests/test_temporal_motion_cpu.py among 4, 8, 16 and 32 (README, "Object history"). */
#define PT_OBJECT_HISTORY_MAX 4.0f

int pt_counters(PtCounters *out);     /* synchronises */
int pt_counters_reset(void);

/* pathtraceFree: tolerant of the never-initialised state (src/main.cpp:91-94 calls it first). */
void pt_free(void);

const char *pt_last_error(void);

/* Number of HIP devices visible (0 = none; the library then refuses to run). */
int pt_device_count(void);

/* ---- stream compaction library (the reference's empty stream_compaction/ stub, README.md:83-86):
 * work-efficient exclusive scan / compaction over DEVICE buffers, multi-block, any n >= 0 (compaction: n < 2^32).
 * Reduce-then-scan over at most 2048 chunks: two launches on `stream`, asynchronous, no workgroup waits for another;
 * calls on different streams use separate workspaces and may overlap.  Sums wrap modulo 2^32 like int32 arithmetic. ---------- */
int pt_scan_exclusive_i32(const int32_t *in_dev, int32_t *out_dev, int64_t n, void *stream);
/* keeps the non-zero elements in order; *count_dev (device) receives how many were kept */
int pt_compact_nonzero_i32(const int32_t *in_dev, int32_t *out_dev, int64_t n, int64_t *count_dev,
                           void *stream);

/* ---- contexts and device groups (round 5) -----------------------------------------------------------------------------------------
 * The reference's renderer is one set of file-static globals bound to device 0 (src/pathtrace.cu:70-71, src/preview.cpp:107).  Here a
 * renderer is a context: pt_ctx_create makes one, pt_ctx_make_current(ctx) makes every function above act on it for the calling thread
 * (NULL: back to the default context), pt_ctx_destroy frees its renderer and the context.  A context initialised on a device makes that
 * device current when it is made current.  pt_set_meshes, pt_set_textures and pt_set_bump_maps register per context. */
typedef struct PtContext PtContext;
PtContext *pt_ctx_create(void);               /* NULL: out of memory */
int        pt_ctx_make_current(PtContext *ctx /* NULL = the default context */);
PtContext *pt_ctx_current(void);              /* NULL = the default context */
int        pt_ctx_destroy(PtContext *ctx);    /* PT_ERR_INVALID while the context is current on ANOTHER thread (that thread's next call
                                                 would act on freed memory); the caller's own current context may be destroyed: the
                                                 thread falls back to the default one.  The current HIP device is left as it was. */

/* A GROUP: n contexts that render the row shards y % n of ONE frame, member i on devices[i] (NULL: device i % pt_device_count()) -- the
 * node's GPUs side by side in one host process ("single process, ncclCommInitAll, one stream per device"; the reference is
 * hard-wired to device 0, src/preview.cpp:107), or several renderers on one device.  Pixels are seeded by their global index, so the shards
 * together are the one-device frame bit for bit.  Every member's launches are enqueued by a host thread of its own.
 *   pt_group_init            = pt_init on every member (opts' shard_rank / shard_count / device / stream / accum_dev are the group's to set;
 *                              max_batch, pipeline_depth, flags and the lens apply to each member).  The members on one device commit their rows
 *                              into ONE zero-padded full-frame accumulator of that device.
 *   pt_group_iterate_batch   enqueues every member's wavefront batch (asynchronous: the devices run concurrently).
 *   pt_group_reduce          assembles the frame from what has been committed so far, asynchronously: members on DISTINCT devices (and
 *                              librccl.so loadable: dlopen, never linked) by ONE ncclReduce(sum, float32, 3 W H, root = member 0's device) over
 *                              xGMI of double-buffered snapshots of the devices' accumulators on a collective stream per device -- the next
 *                              iteration's commits wait on the device for the snapshot only, never for the reduce, and nothing waits on the host.
 *                              A commit writes its member's rows of a snapshot and nothing else, so a snapshot's other rows must stay zero:
 *                              across devices the root receives the sum into a result frame of its own, which pt_group_readback copies
 *                              (the root's snapshot as the receive buffer would add its stale copy of the other devices' rows at every later
 *                              reduce of it); in a one-rank communicator the reduce is the identity and runs on the snapshot itself.
 *                              Members that all share ONE device need no collective (their accumulator is the frame).
 *   pt_group_iterate         = pt_group_iterate_batch(frame, iter, 1) + pt_group_reduce: BASELINE config C3 as written -- the reference's
 *                              per-iteration full-frame transfer (src/pathtrace.cu:170-171, src/main.cpp:97-106) with the reduce in its place.
 *                              With PT_FLAG_TRACE_AHEAD in opts->flags the iteration comes out of batches traced ahead (one small commit per call).
 *   pt_group_readback        the latest assembled frame's running sum on the host (assembling first if commits were enqueued since): one D2H copy
 *                              on the root's collective stream and a wait for THAT stream -- not for the batches traced ahead.
 *   pt_group_sync            waits for every member's streams and the collective streams; reports a member's device fault.
 * pt_group_collective() says how the frame is assembled: "rccl reduce ..." (with "unmeasured across devices": NO multi-GPU node was
 * available to any build round -- the leg has run in a one-rank communicator only), "shared accumulator" (one device) or "host gather"
 * (several devices without RCCL: every device's frame copied to the host, rows taken from their owners; synchronous).
 * PT_AMD_COLLECTIVE=host|rccl overrides (rccl: a one-rank communicator even when every member shares one device);
 * PT_AMD_GROUP_THREADS=0 issues every member's work from the calling thread (experiments).
 * A failed ncclReduce leaves RCCL's call group closed (ncclGroupEnd runs on every path) and the group usable: a later call tries again.
 * A group the host forgets to destroy is destroyed by the library's exit handler. */
typedef struct PtGroup PtGroup;
int  pt_group_create(PtGroup **out, int n, const int32_t *devices /* may be NULL */);
void pt_group_destroy(PtGroup *g);
int  pt_group_size(const PtGroup *g);
const char *pt_group_collective(const PtGroup *g);
int  pt_group_set_meshes(PtGroup *g, const PtMesh *meshes, int nmeshes);
int  pt_group_set_textures(PtGroup *g, const PtTexture *textures, int ntextures, size_t texture_struct_bytes, const PtTexBinding *bindings,
                           int nbindings, size_t binding_struct_bytes);
int  pt_group_set_bump_maps(PtGroup *g, const PtBumpBinding *bindings, int nbindings, size_t binding_struct_bytes);
int  pt_group_init(PtGroup *g, const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth,
                   const PtOptions *opts /* may be NULL */);
int  pt_group_iterate_batch(PtGroup *g, int frame, int first_iter, int count);
int  pt_group_iterate(PtGroup *g, int frame, int iter);
int  pt_group_reduce(PtGroup *g);
int  pt_group_sync(PtGroup *g);
int  pt_group_readback(PtGroup *g, float *rgb_sum_host);
int  pt_group_counters(PtGroup *g, PtCounters *out);      /* summed over the members; iterations: the least any member has committed */

#ifdef __cplusplus
}
#endif
#endif /* PT_AMD_H */
