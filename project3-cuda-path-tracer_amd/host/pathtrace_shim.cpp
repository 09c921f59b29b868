// pathtrace_shim.cpp -- the three reference symbols (src/pathtrace.cu:75-92,123-174) over the C ABI.
// Error behaviour follows checkCUDAError (src/pathtrace.cu:21-39): message on stderr, exit(EXIT_FAILURE).
#include "pathtrace.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_amd.h"

static Scene *hst_scene = NULL;
// PT_AMD_DEVICES=<n> (n >= 2): the frame's rows are rendered by n renderers side by side -- one per HIP device of the node, member i
// on device i % pt_device_count() -- behind the same three symbols (include/pt_amd.h: pt_group_*; the reference is hard-wired to
// device 0, src/preview.cpp:107).  The image after every call is the one-device image bit for bit.  Headless hosts only: a device
// `pbo` belongs to one device's GL context, which a group has none of.
static PtGroup *group = NULL;
static float extraLens = 0.0f, extraFocal = 0.0f;   // README extras (pathtraceExtras), off = the reference's renderer
static bool extraDirect = false;
static bool extraMoments = false;                   // pathtraceMoments: PT_FLAG_MOMENTS for the next pathtraceInit
static bool extraSpatial = false;                   // pathtraceSpatialVariance: PT_FLAG_MOMENTS | PT_FLAG_SPATIAL_VARIANCE for the next pathtraceInit
static bool extraDemod = false;                     // pathtraceDemodulate: PT_FLAG_MOMENTS | PT_FLAG_DEMODULATE for the next pathtraceInit
static bool extraDisplay = false;                   // pathtraceDisplayFilter: PT_FLAG_MOMENTS | PT_FLAG_DISPLAY_FILTER for the next pathtraceInit
static bool extraTemporal = false;                  // pathtraceTemporal: PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL for the next pathtraceInit
static bool extraObjectHistory = false;             // pathtraceObjectHistory: PT_FLAG_OBJECT_HISTORY where the next pathtraceInit sets PT_FLAG_TEMPORAL
static bool extraKeep = false;                      // pathtraceKeepRenderer: pathtraceFree parks the renderer, pathtraceInit sets PT_FLAG_KEEP_RENDERER
// a renderer of the default context exists (a pathtraceInit succeeded and pt_free has not been called since) / pathtraceFree has parked it
static bool live = false, parked = false;

// PT_AMD_KEEP_RENDERER=1 (or pathtraceKeepRenderer(true)): the reference's camera-move restart, pathtraceFree(); pathtraceInit(scene);
// (src/main.cpp:91-95), keeps the renderer.  pathtraceFree only releases the page-locked registration of state.image and PARKS the renderer --
// which goes on holding its device memory between Free and Init: pools, accumulators, tables, streams and events --, and the next pathtraceInit
// calls the full pt_init with PT_FLAG_KEEP_RENDERER, so the library moves the camera in place where the scene, the options and everything
// registered are the parked renderer's own, and runs the full call where they are not (include/pt_amd.h).  The image after every call is the
// same bit for bit.  A parked renderer is freed by a pathtraceFree() called while it is parked, by a pathtraceFree() after the switch was
// turned off, and by the library's exit handler.  The variable, where it is set, decides (0: off whatever the host called).
static bool keepSwitch() {
    if (const char *e = getenv("PT_AMD_KEEP_RENDERER")) return atoi(e) != 0;
    return extraKeep;
}

static void checkPtError(int status, const char *msg) {
    if (status == PT_OK) return;
    fprintf(stderr, "HIP error (pathtrace_shim.cpp): %s: %s\n", msg, pt_last_error());
    exit(EXIT_FAILURE);
}

void pathtraceInit(Scene *scene) {
    hst_scene = scene;
    static_assert(sizeof(Geom) == sizeof(PtGeom) && sizeof(Material) == sizeof(PtMaterial) &&
                  sizeof(Camera) == sizeof(PtCamera), "layout contract of include/pt_amd.h");
    PtOptions opt = PtOptions();        // all defaults = the reference's behaviour ...
    opt.shard_count = 1;
    opt.device = -1;
    opt.lens_radius = extraLens;        // ... unless pathtraceExtras() switched a README extra on
    opt.focal_distance = extraFocal;
    if (extraDirect) opt.flags |= PT_FLAG_DIRECT_LIGHTING;
    if (extraMoments) opt.flags |= PT_FLAG_MOMENTS;
    // PT_AMD_DISPLAY_FILTER=1 (or pathtraceDisplayFilter): the `pbo` of pathtrace receives the variance-guided filter's bytes instead of the raw
    // accumulator's -- for a host built against the reference's header unchanged.  state.image stays the raw sum.
    bool display = extraDisplay;
    if (const char *e = getenv("PT_AMD_DISPLAY_FILTER")) display = display || atoi(e) != 0;
    if (display) opt.flags |= PT_FLAG_MOMENTS | PT_FLAG_DISPLAY_FILTER;
    // PT_AMD_SPATIAL_VARIANCE=1 (or pathtraceSpatialVariance): a pixel with fewer than two samples is filtered under a variance estimated from its
    // neighbours -- with the display filter the `pbo` of the FIRST pathtrace call after an Init is filtered too (the frame a camera drag shows).
    bool spatial = extraSpatial;
    if (const char *e = getenv("PT_AMD_SPATIAL_VARIANCE")) spatial = spatial || atoi(e) != 0;
    if (spatial) opt.flags |= PT_FLAG_MOMENTS | PT_FLAG_SPATIAL_VARIANCE;
    // PT_AMD_DEMODULATE=1 (or pathtraceDemodulate): the variance-guided filter -- pt_denoise_var, and with the display filter the `pbo` -- runs on
    // the frame divided by every pixel's mean first-hit albedo, which is multiplied back behind it: textures survive.  The albedo follows the
    // committed iterations, so such a renderer traces nothing ahead (below).
    bool demod = extraDemod;
    if (const char *e = getenv("PT_AMD_DEMODULATE")) demod = demod || atoi(e) != 0;
    if (demod) opt.flags |= PT_FLAG_MOMENTS | PT_FLAG_DEMODULATE;
    // PT_AMD_TEMPORAL=1 (or pathtraceTemporal): temporal reprojection -- a pathtraceInit over a renderer that was NOT freed keeps the old view's
    // samples as history, which pt_denoise_var and the display filter blend in.  That needs the switch above: without it pathtraceFree frees
    // the renderer and the history with it.  With demodulation the history carries the albedo too.  Such a renderer traces nothing ahead
    // (below): pt_init refuses PT_FLAG_TEMPORAL together with PT_FLAG_TRACE_AHEAD, so every pathtrace call traces its own iteration.
    bool temporal = extraTemporal;
    if (const char *e = getenv("PT_AMD_TEMPORAL")) temporal = temporal || atoi(e) != 0;
    if (temporal) opt.flags |= PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL;
    if (temporal && demod) opt.flags |= PT_FLAG_DEMOD_HISTORY;
    // PT_AMD_OBJECT_HISTORY=1 (or pathtraceObjectHistory), where temporal reprojection is on: the history also survives a pathtraceInit whose
    // scene shows the same objects in other poses, and follows them (include/pt_amd.h: "object history"); any other change of the scene drops it.
    bool objectHistory = extraObjectHistory;
    if (const char *e = getenv("PT_AMD_OBJECT_HISTORY")) objectHistory = objectHistory || atoi(e) != 0;
    if (temporal && objectHistory) opt.flags |= PT_FLAG_OBJECT_HISTORY;
    const bool keep = keepSwitch();
    if (keep) opt.flags |= PT_FLAG_KEEP_RENDERER;
    // The reference's host calls pathtrace(pbo, frame, iter) once per iteration with iter = 1, 2, 3, ... (src/main.cpp:97-103):
    // the library traces such a sequence in wavefront batches AHEAD of the calls (PT_FLAG_TRACE_AHEAD; same image after every
    // call, bit for bit), so a call costs a commit instead of eight small dependent launches.  A camera move goes through
    // pathtraceFree / pathtraceInit (src/main.cpp:91-95), which drops whatever was traced ahead.
    // PT_AMD_TRACE_AHEAD=<iterations per batch> overrides (0 or 1: off, every call traces its own iteration).
    int ahead = 32;
    if (const char *e = getenv("PT_AMD_TRACE_AHEAD")) ahead = atoi(e);
    if (scene->state.iterations < (unsigned)(ahead > 0 ? ahead : 0)) ahead = (int)scene->state.iterations;
    if (ahead > PT_MAX_BATCH) ahead = PT_MAX_BATCH;
    if (demod) ahead = 1;               // (PT_FLAG_DEMODULATE is not for PT_FLAG_TRACE_AHEAD renderers)
    if (temporal) ahead = 1;            // (nor is PT_FLAG_TEMPORAL)
    // A host written against the reference's pathtraceInit knows nothing of batches, so tracing ahead must never be the
    // reason an Init fails: the batch is clamped to the library's limits for this frame (pixels x batch <= 2^29 paths,
    // rows x padded width x batch < 2^30 tile slots: an 8192 x 8192 frame still traces 8 iterations ahead), and should the
    // pools of the batch not fit the device's free memory -- pt_init then fails before it has allocated any -- it is halved
    // until they do; the last resort is the plain protocol, one iteration per call, which fits frames up to 2^30 pixels.
    {
        const long long W = scene->state.camera.resolution.x, H = scene->state.camera.resolution.y;
        const long long padded = (W + 255) / 256 * 256 * H;
        while (ahead > 1 && (W * H * ahead > (1ll << 29) || padded * ahead >= (1ll << 30))) ahead /= 2;
    }
    // `mesh` objects (README.md:236): their triangles go in before the geoms that refer to them.  (Built against the
    // reference's own scene.h, whose loader knows no meshes, the shim registers none.)
    std::vector<PtMesh> meshes;
#ifdef PT_SCENE_HAS_MESHES
    for (size_t i = 0; i < scene->meshes.size(); ++i) {
        PtMesh m;
        m.geom = scene->meshes[i].geom;
        m.ntris = (int)(scene->meshes[i].tris.size() / 9);
        m.tris = scene->meshes[i].tris.data();
        m.normals = scene->meshes[i].normals.empty() ? NULL : scene->meshes[i].normals.data();      // `vn`: smooth shading
        m.materials = scene->meshes[i].mats.empty() ? NULL : scene->meshes[i].mats.data();          // `usemtl <k>`: a material per face
        meshes.push_back(m);
    }
#endif
    // `TEXTURE <file>` lines: the scene's textures, and per textured object its binding (a mesh's with its corner UVs)
    std::vector<PtTexture> textures;
    std::vector<PtTexBinding> bindings;
#ifdef PT_SCENE_HAS_TEXTURES
    for (size_t i = 0; i < scene->textures.size(); ++i) {
        PtTexture t;
        t.width = scene->textures[i].width;
        t.height = scene->textures[i].height;
        t.rgb = scene->textures[i].rgb.data();
        textures.push_back(t);
    }
    for (size_t g = 0; g < scene->geomTextures.size(); ++g) {
        if (scene->geomTextures[g] < 0) continue;
        PtTexBinding b;
        b.geom = (int)g;
        b.texture = scene->geomTextures[g];
        b.ntris = 0;
        b.uvs = NULL;
        for (size_t i = 0; i < scene->meshes.size(); ++i)
            if (scene->meshes[i].geom == (int)g) {
                b.ntris = (int)(scene->meshes[i].tris.size() / 9);
                b.uvs = scene->meshes[i].uvs.empty() ? NULL : scene->meshes[i].uvs.data();
            }
        bindings.push_back(b);
    }
#endif
    // `BUMP <file> <scale>` lines: per bump-mapped object its height map (one of the textures above), its scale and a mesh's corner UVs
    std::vector<PtBumpBinding> bumps;
#ifdef PT_SCENE_HAS_BUMPS
    for (size_t g = 0; g < scene->geomBumps.size(); ++g) {
        if (scene->geomBumps[g] < 0) continue;
        PtBumpBinding b;
        b.geom = (int)g;
        b.texture = scene->geomBumps[g];
        b.scale = scene->bumpScales[g];
        b.ntris = 0;
        b.uvs = NULL;
        for (size_t i = 0; i < scene->meshes.size(); ++i)
            if (scene->meshes[i].geom == (int)g) {
                b.ntris = (int)(scene->meshes[i].tris.size() / 9);
                b.uvs = scene->meshes[i].uvs.empty() ? NULL : scene->meshes[i].uvs.data();
            }
        bumps.push_back(b);
    }
#endif
    int members = 1;
    if (const char *e = getenv("PT_AMD_DEVICES")) members = atoi(e);
    if (members >= 2 && spatial) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: the spatial variance estimate (PT_AMD_SPATIAL_VARIANCE, pathtraceSpatialVariance) "
                        "is not for PT_AMD_DEVICES: a group keeps no second moments\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2 && demod) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: demodulation (PT_AMD_DEMODULATE, pathtraceDemodulate) is not for PT_AMD_DEVICES: "
                        "a group keeps no second moments\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2 && display) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: the display filter (PT_AMD_DISPLAY_FILTER, pathtraceDisplayFilter) is not for "
                        "PT_AMD_DEVICES: a group renders headless\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2 && temporal) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: temporal reprojection (PT_AMD_TEMPORAL, pathtraceTemporal) is not for PT_AMD_DEVICES: "
                        "a group keeps no second moments\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2 && objectHistory) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: object history (PT_AMD_OBJECT_HISTORY, pathtraceObjectHistory) is not for "
                        "PT_AMD_DEVICES: a group keeps no history\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2 && keep) {
        fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtraceInit: keeping the renderer (PT_AMD_KEEP_RENDERER, pathtraceKeepRenderer) is not for "
                        "PT_AMD_DEVICES: a group re-initialises its members in place already\n");
        exit(EXIT_FAILURE);
    }
    if (members >= 2) {
        if (parked) {                   // (a renderer parked before PT_AMD_DEVICES was set: the group takes its place)
            pt_free();
            live = parked = false;
        }
        if (group && pt_group_size(group) != members) {
            pt_group_destroy(group);
            group = NULL;
        }
        if (!group) checkPtError(pt_group_create(&group, members, NULL), "pathtraceInit (PT_AMD_DEVICES)");
        checkPtError(pt_group_set_meshes(group, meshes.empty() ? NULL : meshes.data(), (int)meshes.size()), "pathtraceInit");
        checkPtError(pt_group_set_textures(group, textures.empty() ? NULL : textures.data(), (int)textures.size(), sizeof(PtTexture),
                                           bindings.empty() ? NULL : bindings.data(), (int)bindings.size(), sizeof(PtTexBinding)), "pathtraceInit");
        checkPtError(pt_group_set_bump_maps(group, bumps.empty() ? NULL : bumps.data(), (int)bumps.size(), sizeof(PtBumpBinding)), "pathtraceInit");
    } else {
        checkPtError(pt_set_meshes_sized(meshes.empty() ? NULL : meshes.data(), (int)meshes.size(), sizeof(PtMesh)), "pathtraceInit");
        checkPtError(pt_set_textures(textures.empty() ? NULL : textures.data(), (int)textures.size(), sizeof(PtTexture),
                                     bindings.empty() ? NULL : bindings.data(), (int)bindings.size(), sizeof(PtTexBinding)), "pathtraceInit");
        checkPtError(pt_set_bump_maps(bumps.empty() ? NULL : bumps.data(), (int)bumps.size(), sizeof(PtBumpBinding)), "pathtraceInit");
    }
    int status;
    for (;;) {
        opt.flags &= ~PT_FLAG_TRACE_AHEAD;
        opt.max_batch = 0;
        opt.pipeline_depth = 0;
        if (ahead > 1) {
            opt.flags |= PT_FLAG_TRACE_AHEAD;
            opt.max_batch = ahead;
            opt.pipeline_depth = 2;     // one batch being consumed, one being traced (a third in flight only competes with the copy)
        }
        const PtCamera *cam = reinterpret_cast<const PtCamera *>(&scene->state.camera);
        const PtGeom *geoms = reinterpret_cast<const PtGeom *>(scene->geoms.data());
        const PtMaterial *mats = reinterpret_cast<const PtMaterial *>(scene->materials.data());
        status = group ? pt_group_init(group, cam, geoms, (int)scene->geoms.size(), mats, (int)scene->materials.size(), scene->state.traceDepth, &opt)
                       : pt_init(cam, geoms, (int)scene->geoms.size(), mats, (int)scene->materials.size(), scene->state.traceDepth, &opt);
        // (PT_ERR_INVALID / PT_ERR_HIP: a limit or an allocation that a smaller batch may satisfy; anything else is final)
        if (status == PT_OK || ahead <= 1 || (status != PT_ERR_INVALID && status != PT_ERR_HIP)) break;
        ahead /= 2;
    }
    checkPtError(status, "pathtraceInit");
    live = !group;
    parked = false;
    // state.image is owned by the Scene and lives from Init to Free: page-lock it for the per-iteration copy below
    // (an optimisation only; failure to register is not an error of the renderer)
    // (a group's read-back copies into the same buffer: the registration is process-wide, made through the default context)
    if (!scene->state.image.empty())
        (void)pt_pin_host(scene->state.image.data(), scene->state.image.size() * sizeof(scene->state.image[0]));
}

// Not a reference symbol: depth of field and direct lighting (README.md:100-101, :107-108) for the next pathtraceInit.
// A host that never calls it gets exactly the reference's renderer.
void pathtraceExtras(float lensRadius, float focalDistance, bool directLighting) {
    extraLens = lensRadius;
    extraFocal = focalDistance;
    extraDirect = directLighting;
}

// Not a reference symbol either: the next pathtraceInit also keeps the samples' second moments (PT_FLAG_MOMENTS: pt_variance,
// pt_denoise_var).  Not with PT_AMD_DEVICES: a group refuses the flag.
void pathtraceMoments(bool on) { extraMoments = on; }

// ... nor this one: the next pathtraceInit sets PT_FLAG_MOMENTS | PT_FLAG_DISPLAY_FILTER, and the `pbo` of every pathtrace call from the second
// iteration on receives the bytes of the variance-guided filter (include/pt_amd.h: "display filter"), made on the device behind the commit.
// The environment variable PT_AMD_DISPLAY_FILTER=1 does the same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceDisplayFilter(bool on) { extraDisplay = on; }

// ... nor this one: the next pathtraceInit sets PT_FLAG_MOMENTS | PT_FLAG_SPATIAL_VARIANCE (include/pt_amd.h: "spatial variance"): pt_denoise_var accepts
// one sample, and with the display filter the first frame's `pbo` is filtered as well.  The environment variable PT_AMD_SPATIAL_VARIANCE=1 does the
// same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceSpatialVariance(bool on) { extraSpatial = on; }

// ... nor this one: the next pathtraceInit sets PT_FLAG_MOMENTS | PT_FLAG_DEMODULATE (include/pt_amd.h: "demodulation") and traces nothing ahead.
// The environment variable PT_AMD_DEMODULATE=1 does the same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceDemodulate(bool on) { extraDemod = on; }

// ... nor this one: the next pathtraceInit sets PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL (include/pt_amd.h: "temporal reprojection"; with demodulation
// PT_FLAG_DEMOD_HISTORY too) and traces nothing ahead.  History passes a pathtraceFree only with pathtraceKeepRenderer.  The environment variable
// PT_AMD_TEMPORAL=1 does the same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceTemporal(bool on) { extraTemporal = on; }

// ... nor this one: pathtraceFree parks the renderer instead of freeing it, and pathtraceInit lets the library move the camera in place
// (keepSwitch above).  The environment variable PT_AMD_KEEP_RENDERER=1 does the same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceKeepRenderer(bool on) { extraKeep = on; }
// ... and where temporal reprojection is on, the next pathtraceInit sets PT_FLAG_OBJECT_HISTORY too (include/pt_amd.h: "object history"): a
// scene that shows the same objects in other poses keeps the history, which follows them.  The environment variable PT_AMD_OBJECT_HISTORY=1
// does the same for a host that cannot call it.  Not with PT_AMD_DEVICES.
void pathtraceObjectHistory(bool on) { extraObjectHistory = on; }

void pathtraceFree() {
    if (group) {
        pt_group_destroy(group);
        group = NULL;
    }
    if (live && !parked && keepSwitch()) {
        // state.image belongs to the host again (it may resize or release it before the next Init); everything else stays
        checkPtError(pt_unpin_host(), "pathtraceFree");
        parked = true;
        return;
    }
    live = parked = false;
    pt_free();  // no-op when nothing was initialised (src/main.cpp:91-94 calls Free before the first Init)
}

void pathtrace(uchar4 *pbo, int frame, int iter) {
    if (group) {
        if (pbo) {
            fprintf(stderr, "HIP error (pathtrace_shim.cpp): pathtrace: PT_AMD_DEVICES renders headless (pbo must be NULL)\n");
            exit(EXIT_FAILURE);
        }
        // one iteration on every member and the frame's reduce (asynchronous: the members go on tracing ahead), then the copy of the
        // reduced frame, which waits for the collective stream alone
        checkPtError(pt_group_iterate(group, frame, iter), "pathtrace");
        checkPtError(pt_group_readback(group, reinterpret_cast<float *>(hst_scene->state.image.data())), "pathtrace");
        return;
    }
    checkPtError(pt_iterate(frame, iter, pbo), "pathtrace");
    // Retrieve image from GPU: the un-normalised running sum (src/pathtrace.cu:170-171)
    checkPtError(pt_readback(reinterpret_cast<float *>(hst_scene->state.image.data())), "pathtrace");
}
