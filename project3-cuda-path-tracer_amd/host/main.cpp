// main.cpp -- headless driver: the reference's main()/runCuda()/saveImage() without GLFW/GL
// (reference src/main.cpp:21-113).  Same protocol: Free -> Init when iteration == 0, 1-based
// iteration passed to pathtrace(pbo, 0, iteration), save + Free when the sample count is reached,
// output name <FILE>.<start time>.<N>samp.png, X mirrored, divided by the sample count.
//
//   pt_render SCENEFILE.txt [--res W H] [--iterations N] [--depth D] [--out BASENAME] [--hdr] [--batch B]
//                           [--lens RADIUS FOCALDISTANCE] [--direct] [--denoise LEVELS SIGMACOLOR SIGMANORMAL SIGMAPOSITION]
//                           [--denoise-var LEVELS SIGMALUM SIGMANORMAL SIGMAPOSITION]
//                           [--noise-threshold T [--noise-fraction F] [--check-every K]]
//                           [--history-from EX EY EZ N [--in-place | --protocol]] [--spatial-variance] [--demodulate] [--history-albedo]
//                           [--no-motion]
// --lens / --direct switch on the README extras (depth of field, README.md:100-101; direct lighting, :107-108);
// imperfect specular needs no switch, it is a material's SPECEX > 0 in the scene file (README.md:171-185).
// --denoise also writes <out>.denoised.png: the same frame through pt_denoise, the edge-avoiding a-trous filter guided by the first
// iteration's first hits (include/pt_amd.h); the usual image is written as without the option.
// --denoise-var writes the same file through pt_denoise_var, the variance-guided filter: the renderer then runs with PT_FLAG_MOMENTS.
// One of the two at most.
// --noise-threshold T renders until no 16 x 16 tile's relative standard error lies above T (pt_iterate_until, include/pt_amd.h) -- with
// --noise-fraction F until at most that fraction of the tiles does -- checking every K iterations (--check-every, default 8) while the next
// K are already being traced; --iterations becomes the cap.  The renderer then runs with PT_FLAG_MOMENTS through the C ABI like --batch
// (B may be 1), the PNG is normalised by the samples actually taken, and one line reports them.
// --history-from EX EY EZ N (with --denoise-var) is the camera move of an interactive session, headless: N iterations are rendered from the
// eye (EX, EY, EZ) first, the renderer is then re-initialised at the scene's camera WITHOUT being freed -- both with PT_FLAG_TEMPORAL, so the
// first view's samples become the context's history (include/pt_amd.h, "temporal reprojection") --, --iterations more are rendered there
// (numbered N + 1, ...: fresh random numbers), and <out>.denoised.png is the filter of the blend.  The usual image holds the second view's
// own samples alone.  Through the C ABI like --noise-threshold (B may be 1); not together with it.
// --in-place makes that move by pt_init's same-scene form (PT_SAME_SCENE), which keeps the renderer's buffers.  --protocol makes it the way
// the reference's host does -- pathtraceFree(); pathtraceInit(scene); (src/main.cpp:91-95) -- through the shim's three symbols, one pathtrace
// call per iteration, with pathtraceKeepRenderer and pathtraceTemporal switched on: Free parks the renderer, Init moves its camera in place
// (PT_FLAG_KEEP_RENDERER).  The same PNGs, byte for byte, all three ways.  One of the two at most.
// --spatial-variance (with --denoise-var) runs the renderer with PT_FLAG_SPATIAL_VARIANCE: a pixel with fewer than two effective samples is
// filtered under a variance estimated from its neighbours (include/pt_amd.h, "spatial variance"), so --iterations 1 is allowed, and with
// --history-from a new view of one sample.
// --demodulate (with --denoise-var; not with --history-from) runs the renderer with PT_FLAG_DEMODULATE: <out>.denoised.png is the filter of the
// frame divided by every pixel's mean first-hit albedo, multiplied back behind it (include/pt_amd.h, "demodulation").
// --history-move ID TX TY TZ [RX RY RZ] (with --denoise-var and --history-from) runs both renderers with PT_FLAG_OBJECT_HISTORY, and the history
// view renders object ID displaced by that translation (and rotation, in degrees) from the scene file's pose; the final view renders the
// file's pose, and its history follows the object (include/pt_amd.h, "object history").
// --history-albedo (with --denoise-var and --history-from) runs both renderers with PT_FLAG_TEMPORAL, PT_FLAG_DEMODULATE and
// PT_FLAG_DEMOD_HISTORY: the history carries the first view's albedo, and <out>.denoised.png is the filter of the blend divided by the blended
// albedo (include/pt_amd.h, "demodulated history").
// A scene whose OBJECT blocks carry TRANS_END / ROTAT_END / SCALE_END (scene.h: Scene::stepGeoms) is rendered motion-blurred: through the C
// ABI like --noise-threshold (B may be 1) with PT_FLAG_MOTION and the loader's 16 poses (include/pt_amd.h, "motion blur"); the scene's
// textures and height maps are registered with it.  Not with --denoise, --denoise-var or --history-from.  --no-motion renders the scene of step 0 instead,
// static, every way a scene without the keywords is rendered.
//
// --batch B (B > 1) leaves the reference protocol where nothing can observe it: iterations are traced B at a time
// through the C ABI (pt_iterate_batch) and the running sum is copied to the host once, before the image is saved,
// instead of after every iteration.  Same pixels (bit for bit), an order of magnitude less wall time.
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstring>
#include <ctime>
#include <sstream>
#include <stdexcept>

#include "image.h"
#include "pathtrace.h"
#include "pt_amd.h"
#include "utilities.h"

static std::string startTimeString;
static Scene *scene;
static RenderState *renderState;
static int iteration;
static int width, height;
static std::string outBase;
static bool writeHdr = false;
static int batch = 1;
static float lensRadius = 0.0f, focalDistance = 0.0f;
static bool directLighting = false;
static PtDenoiseParams denoiseParams;
static bool denoise = false;
static PtDenoiseVarParams denoiseVarParams;
static bool denoiseVar = false;
static bool noiseTarget = false;
static float noiseThreshold = 0.0f, noiseFraction = 0.0f;
static int checkEvery = 8;
static bool historyFrom = false;
static bool inPlace = false;         // --in-place (with --history-from): the move is made by pt_init's same-scene form
static bool protocol = false;        // --protocol (with --history-from): the move is made by pathtraceFree(); pathtraceInit(scene); through the shim
static float historyEye[3] = {0.0f, 0.0f, 0.0f};
static int historyIterations = 0;
static bool spatialVariance = false;
static bool demodulate = false;
static bool historyAlbedo = false;
static bool historyMove = false;     // --history-move (with --history-from): the history view shows object historyMoveId in another pose
static int historyMoveId = 0;
static float historyMoveT[3] = {0.0f, 0.0f, 0.0f}, historyMoveR[3] = {0.0f, 0.0f, 0.0f};
static bool noMotion = false;        // --no-motion: a scene that defines motion is rendered in step 0's pose
static bool motion = false;          // the scene defines motion and --no-motion was not given: PT_FLAG_MOTION with Scene::stepGeoms
void pathtraceExtras(float lensRadius, float focalDistance, bool directLighting);   // pathtrace_shim.cpp
void pathtraceMoments(bool on);                                                     // pathtrace_shim.cpp
void pathtraceSpatialVariance(bool on);                                             // pathtrace_shim.cpp
void pathtraceDemodulate(bool on);                                                  // pathtrace_shim.cpp
// (pathtraceTemporal, pathtraceKeepRenderer: pathtrace.h)

static std::string currentTimeString() {
    time_t now;
    time(&now);
    char buf[sizeof "0000-00-00_00-00-00z"];
    strftime(buf, sizeof buf, "%Y-%m-%d_%H-%M-%Sz", gmtime(&now));
    return std::string(buf);
}

static void saveImage() {
    float samples = iteration;
    image img(width, height);
    for (int x = 0; x < width; x++) {
        for (int y = 0; y < height; y++) {
            int index = x + (y * width);
            lin::vec3 pix = renderState->image[index];
            img.setPixel(width - 1 - x, y, pix / samples);   // X mirror, src/main.cpp:58
        }
    }
    std::ostringstream ss;
    if (outBase.empty()) ss << renderState->imageName << "." << startTimeString << "." << samples << "samp";
    else ss << outBase;
    img.savePNG(ss.str());
    if (writeHdr) img.saveHDR(ss.str());   // the reference keeps this behind a comment, src/main.cpp:69
}

static void check(int status, const char *what);
// --denoise: the filtered mean, before the renderer is freed
static void saveDenoised() {
    if (!denoise && !denoiseVar) return;
    std::vector<lin::vec3> mean((size_t)width * height);
    if (denoise) check(pt_denoise(iteration, &denoiseParams, sizeof denoiseParams, (float *)mean.data()), "pt_denoise");
    else check(pt_denoise_var(iteration, &denoiseVarParams, sizeof denoiseVarParams, (float *)mean.data(), NULL), "pt_denoise_var");
    image img(width, height);
    for (int x = 0; x < width; x++)
        for (int y = 0; y < height; y++) img.setPixel(width - 1 - x, y, mean[x + (y * width)]);
    std::ostringstream ss;
    if (outBase.empty()) ss << renderState->imageName << "." << startTimeString << "." << (float)iteration << "samp";
    else ss << outBase;
    ss << ".denoised";
    img.savePNG(ss.str());
}

// one trip through the reference's per-frame function; returns false when rendering is complete
static bool runHip() {
    if (iteration == 0) {
        pathtraceFree();
        pathtraceInit(scene);
    }
    if (iteration < (int)renderState->iterations) {
        iteration++;
        pathtrace(NULL, 0, iteration);   // headless: no PBO
        return true;
    }
    saveImage();
    saveDenoised();
    pathtraceFree();
    return false;
}

// --batch: pt_init / pt_iterate_batch / pt_readback directly; exits like checkCUDAError on a failure
static void check(int status, const char *what) {
    if (status == PT_OK) return;
    fprintf(stderr, "HIP error (main.cpp): %s: %s\n", what, pt_last_error());
    exit(EXIT_FAILURE);
}
static void renderBatched() {
    PtOptions opt;
    memset(&opt, 0, sizeof opt);
    opt.shard_count = 1;
    opt.device = -1;
    opt.max_batch = batch;
    opt.pipeline_depth = 2;        // two batches in flight are as fast as three and provision a third less memory
    opt.lens_radius = lensRadius;
    opt.focal_distance = focalDistance;
    if (directLighting) opt.flags |= PT_FLAG_DIRECT_LIGHTING;
    if (denoiseVar || noiseTarget) opt.flags |= PT_FLAG_MOMENTS;
    if (historyFrom) opt.flags |= PT_FLAG_TEMPORAL;
    if (spatialVariance) opt.flags |= PT_FLAG_SPATIAL_VARIANCE;
    if (demodulate) opt.flags |= PT_FLAG_DEMODULATE;
    if (historyAlbedo) opt.flags |= PT_FLAG_DEMODULATE | PT_FLAG_DEMOD_HISTORY;      // (PT_FLAG_MOMENTS and PT_FLAG_TEMPORAL: set above, it needs both options)
    if (historyMove) opt.flags |= PT_FLAG_OBJECT_HISTORY;
    if (motion) opt.flags |= PT_FLAG_MOTION;
    std::vector<PtMesh> meshes;        // `mesh` objects: their triangles first (like pathtrace_shim.cpp)
    for (size_t i = 0; i < scene->meshes.size(); ++i) {
        PtMesh m;
        m.geom = scene->meshes[i].geom;
        m.ntris = (int)(scene->meshes[i].tris.size() / 9);
        m.tris = scene->meshes[i].tris.data();
        m.normals = scene->meshes[i].normals.empty() ? NULL : scene->meshes[i].normals.data();      // `vn`: smooth shading
        m.materials = scene->meshes[i].mats.empty() ? NULL : scene->meshes[i].mats.data();          // `usemtl <k>`: a material per face
        meshes.push_back(m);
    }
    check(pt_set_meshes(meshes.empty() ? NULL : meshes.data(), (int)meshes.size()), "pt_set_meshes");
    // --history-albedo: the scene's textures and their bindings too (like pathtrace_shim.cpp) -- the albedo the history carries is theirs.
    // (Every other run through here registers none, as before.)
    std::vector<PtTexture> textures;
    std::vector<PtTexBinding> bindings;
    if (historyAlbedo || motion) {
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
        check(pt_set_textures(textures.empty() ? NULL : textures.data(), (int)textures.size(), sizeof(PtTexture),
                              bindings.empty() ? NULL : bindings.data(), (int)bindings.size(), sizeof(PtTexBinding)), "pt_set_textures");
    }
    // a scene in motion: its height maps too (like pathtrace_shim.cpp) -- what is registered applies to geom g of every step, and the frame
    // is the Python path's.  (Every other run through here registers none, as before.)
    std::vector<PtBumpBinding> bumps;
    if (motion) {
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
        check(pt_set_bump_maps(bumps.empty() ? NULL : bumps.data(), (int)bumps.size(), sizeof(PtBumpBinding)), "pt_set_bump_maps");
    }
    int firstIter = 1;                 // the iteration number of the frame's first sample
    if (historyFrom) {                 // the view before the camera moved: its samples stay behind as the context's history
        PtCamera before;
        memcpy(&before, &renderState->camera, sizeof before);
        before.position.x = historyEye[0]; before.position.y = historyEye[1]; before.position.z = historyEye[2];
        std::vector<Geom> geomsBefore = scene->geoms;       // --history-move: one object in the pose it had before
        if (historyMove) {
            Geom &g = geomsBefore[(size_t)historyMoveId];
            g.translation = lin::vec3(g.translation.x + historyMoveT[0], g.translation.y + historyMoveT[1], g.translation.z + historyMoveT[2]);
            g.rotation = lin::vec3(g.rotation.x + historyMoveR[0], g.rotation.y + historyMoveR[1], g.rotation.z + historyMoveR[2]);
            g.transform = utilityCore::buildTransformationMatrix(g.translation, g.rotation, g.scale);
            g.inverseTransform = lin::inverse(g.transform);
            g.invTranspose = lin::inverseTranspose(g.transform);
        }
        check(pt_init(&before, (const PtGeom *)geomsBefore.data(), (int)geomsBefore.size(), (const PtMaterial *)scene->materials.data(),
                      (int)scene->materials.size(), renderState->traceDepth, &opt), "pt_init");
        for (int done = 0; done < historyIterations;) {
            const int n = historyIterations - done < batch ? historyIterations - done : batch;
            check(pt_iterate_batch(0, done + 1, n, NULL), "pt_iterate_batch");
            done += n;
        }
        firstIter = historyIterations + 1;
    }
    // (with --history-from: over the live renderer -- no pt_free -- which is what carries the history; --in-place: the same move by
    // pt_init's same-scene form (PT_SAME_SCENE), which keeps the renderer's buffers -- the same PNGs)
    if (historyFrom && inPlace) check(pt_init((const PtCamera *)&renderState->camera, NULL, 0, NULL, 0, PT_SAME_SCENE, NULL), "pt_init (camera move)");
    else
    check(pt_init((const PtCamera *)&renderState->camera, (const PtGeom *)(motion ? scene->stepGeoms.data() : scene->geoms.data()), (int)scene->geoms.size(),
                  (const PtMaterial *)scene->materials.data(), (int)scene->materials.size(), renderState->traceDepth, &opt),
          "pt_init");
    const int total = (int)renderState->iterations;
    if (noiseTarget) {
        PtNoiseTarget t;
        t.threshold = noiseThreshold;
        t.lum_floor = 0.05f;
        t.max_unconverged_fraction = noiseFraction;
        t.min_samples = 2;
        t.max_samples = total;
        t.check_every = checkEvery;
        t.lookahead = 1;
        PtNoiseStats st;
        int32_t done = 0;
        check(pt_iterate_until(0, 1, &t, sizeof t, &st, &done), "pt_iterate_until");
        iteration = done;
        printf("noise threshold %g: %d samples, converged %s, %lld of %lld tiles above it, largest relative standard error %.4f\n", noiseThreshold,
               iteration, st.converged ? "yes" : "no", (long long)st.unconverged, (long long)st.tiles, sqrt((double)st.max_rel_var));
    }
    while (!noiseTarget && iteration < total) {
        const int n = total - iteration < batch ? total - iteration : batch;
        check(pt_iterate_batch(0, firstIter + iteration, n, NULL), "pt_iterate_batch");
        iteration += n;
    }
    check(pt_readback((float *)renderState->image.data()), "pt_readback");
    saveImage();
    saveDenoised();
    pt_free();
}

// --history-from ... --protocol: the two views of renderBatched's --history-from as a host on the reference's three symbols renders them.
// What is registered is what renderBatched registers -- the meshes; the textures under --history-albedo alone; no height map --, so the shim
// is handed the scene without the rest.
static void renderProtocol() {
    if (!historyAlbedo) {
        scene->textures.clear();
        scene->geomTextures.assign(scene->geoms.size(), -1);
    }
    scene->geomBumps.assign(scene->geoms.size(), -1);
    pathtraceKeepRenderer(true);
    pathtraceTemporal(true);
    if (historyAlbedo) pathtraceDemodulate(true);
    const Camera after = renderState->camera;
    PtCamera *cam = (PtCamera *)&renderState->camera;
    cam->position.x = historyEye[0]; cam->position.y = historyEye[1]; cam->position.z = historyEye[2];
    pathtraceFree();
    pathtraceInit(scene);
    for (int i = 1; i <= historyIterations; ++i) pathtrace(NULL, 0, i);
    renderState->camera = after;        // the camera moved: the reference's restart
    pathtraceFree();
    pathtraceInit(scene);
    const int total = (int)renderState->iterations;
    while (iteration < total) {
        iteration++;
        pathtrace(NULL, 0, historyIterations + iteration);
    }
    saveImage();
    saveDenoised();
    pathtraceFree();                    // (parks; the library's exit handler frees)
}

// a token that is a number from its first character to its last
static bool wholeNumber(const char *s, float *out) {
    char *end = NULL;
    const double v = strtod(s, &end);
    if (end == s || *end != '\0') return false;
    *out = (float)v;
    return true;
}

int main(int argc, char **argv) {
    startTimeString = currentTimeString();
    if (argc < 2) {
        printf("Usage: %s SCENEFILE.txt [--res W H] [--iterations N] [--depth D] [--out BASENAME] [--hdr] [--batch B] [--lens R F] [--direct] [--denoise LEVELS SC SN SP | --denoise-var LEVELS SL SN SP] [--noise-threshold T [--noise-fraction F] [--check-every K]] [--history-from EX EY EZ N [--in-place | --protocol]] [--spatial-variance] [--demodulate] [--history-albedo] [--history-move ID TX TY TZ [RX RY RZ]] [--no-motion]\n", argv[0]);
        return 1;
    }
    try {
        scene = new Scene(argv[1], true);
    } catch (const std::exception &e) {          // unreadable scene file, or a mesh object whose OBJ cannot be read
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    renderState = &scene->state;
    for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--res") && i + 2 < argc) { scene->setResolution(atoi(argv[i + 1]), atoi(argv[i + 2])); i += 2; }
        else if (!strcmp(argv[i], "--iterations") && i + 1 < argc) renderState->iterations = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--depth") && i + 1 < argc) renderState->traceDepth = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) outBase = argv[++i];
        else if (!strcmp(argv[i], "--hdr")) writeHdr = true;
        else if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--lens") && i + 2 < argc) { lensRadius = (float)atof(argv[i + 1]); focalDistance = (float)atof(argv[i + 2]); i += 2; }
        else if (!strcmp(argv[i], "--direct")) directLighting = true;
        else if (!strcmp(argv[i], "--denoise") && i + 4 < argc) {
            denoise = true;
            denoiseParams.levels = atoi(argv[i + 1]);
            denoiseParams.guide_iter = 1;
            denoiseParams.sigma_color = (float)atof(argv[i + 2]);
            denoiseParams.sigma_normal = (float)atof(argv[i + 3]);
            denoiseParams.sigma_position = (float)atof(argv[i + 4]);
            i += 4;
        }
        else if (!strcmp(argv[i], "--denoise-var") && i + 4 < argc) {
            denoiseVar = true;
            denoiseVarParams.levels = atoi(argv[i + 1]);
            denoiseVarParams.guide_iter = 1;
            denoiseVarParams.sigma_lum = (float)atof(argv[i + 2]);
            denoiseVarParams.sigma_normal = (float)atof(argv[i + 3]);
            denoiseVarParams.sigma_position = (float)atof(argv[i + 4]);
            i += 4;
        }
        else if (!strcmp(argv[i], "--noise-threshold") && i + 1 < argc) { noiseTarget = true; noiseThreshold = (float)atof(argv[++i]); }
        else if (!strcmp(argv[i], "--noise-fraction") && i + 1 < argc) noiseFraction = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--check-every") && i + 1 < argc) checkEvery = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--in-place")) inPlace = true;
        else if (!strcmp(argv[i], "--protocol")) protocol = true;
        else if (!strcmp(argv[i], "--history-from") && i + 4 < argc) {
            historyFrom = true;
            for (int a = 0; a < 3; ++a) historyEye[a] = (float)atof(argv[i + 1 + a]);
            historyIterations = atoi(argv[i + 4]);
            i += 4;
        }
        else if (!strcmp(argv[i], "--spatial-variance")) spatialVariance = true;
        else if (!strcmp(argv[i], "--demodulate")) demodulate = true;
        else if (!strcmp(argv[i], "--history-albedo")) historyAlbedo = true;
        else if (!strcmp(argv[i], "--no-motion")) noMotion = true;
        else if (!strcmp(argv[i], "--history-move") && i + 4 < argc) {
            historyMove = true;
            float id = 0.0f;
            bool ok = wholeNumber(argv[i + 1], &id) && id == (float)(int)id;
            historyMoveId = (int)id;
            for (int a = 0; a < 3; ++a) ok = wholeNumber(argv[i + 2 + a], &historyMoveT[a]) && ok;
            if (!ok) { fprintf(stderr, "--history-move ID TX TY TZ [RX RY RZ]: ID, TX, TY and TZ must be numbers\n"); return 1; }
            i += 4;
            // the rotation: all three of the next tokens are numbers, or none of them is read
            float r[3];
            if (i + 3 < argc && wholeNumber(argv[i + 1], &r[0]) && wholeNumber(argv[i + 2], &r[1]) && wholeNumber(argv[i + 3], &r[2])) {
                for (int a = 0; a < 3; ++a) historyMoveR[a] = r[a];
                i += 3;
            }
        }
        else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 1; }
    }
    if (denoise && denoiseVar) { fprintf(stderr, "--denoise and --denoise-var exclude each other\n"); return 1; }
    if (historyAlbedo && (!denoiseVar || !historyFrom)) { fprintf(stderr, "--history-albedo needs --denoise-var and --history-from\n"); return 1; }
    if (historyFrom && (!denoiseVar || noiseTarget || historyIterations < 1)) {
        fprintf(stderr, "--history-from needs --denoise-var and N >= 1, and does not go with --noise-threshold\n");
        return 1;
    }
    if (spatialVariance && !denoiseVar) { fprintf(stderr, "--spatial-variance needs --denoise-var\n"); return 1; }
    pathtraceExtras(lensRadius, focalDistance, directLighting);
    pathtraceMoments(denoiseVar);
    if (historyMove && (!denoiseVar || !historyFrom || inPlace || protocol || historyMoveId < 0 || historyMoveId >= (int)scene->geoms.size())) {
        fprintf(stderr, "--history-move needs --denoise-var, --history-from and an object of the scene, and goes with neither --in-place nor --protocol\n");
        return 1;
    }
    if (inPlace && !historyFrom) { fprintf(stderr, "--in-place needs --history-from\n"); return 1; }
    if (protocol && !historyFrom) { fprintf(stderr, "--protocol needs --history-from\n"); return 1; }
    if (protocol && inPlace) { fprintf(stderr, "--protocol and --in-place exclude each other\n"); return 1; }
    if (demodulate && (!denoiseVar || historyFrom)) { fprintf(stderr, "--demodulate needs --denoise-var and does not go with --history-from\n"); return 1; }
    pathtraceSpatialVariance(spatialVariance);
    pathtraceDemodulate(demodulate);
    if (scene->hasMotion() && noMotion) {        // step 0's scene, static
        scene->geoms.assign(scene->stepGeoms.begin(), scene->stepGeoms.begin() + scene->geoms.size());
        scene->stepGeoms.clear();
    }
    motion = scene->hasMotion();
    if (motion && (denoise || denoiseVar || historyFrom)) {
        fprintf(stderr, "a scene with motion (TRANS_END / ROTAT_END / SCALE_END) does not go with --denoise, --denoise-var or --history-from: --no-motion renders it static\n");
        return 1;
    }
    iteration = 0;
    width = renderState->camera.resolution.x;
    height = renderState->camera.resolution.y;
    const auto t0 = std::chrono::steady_clock::now();
    if (protocol) renderProtocol();
    else if (batch > 1 || noiseTarget || historyFrom || motion) renderBatched();
    else while (runHip()) {}
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%d iterations of %dx%d, depth %d: %.3f s wall (init, %s and PNG included)\n", iteration, width, height,
           renderState->traceDepth, s, !protocol && (batch > 1 || noiseTarget || historyFrom || motion) ? "one D2H copy" : "per-iteration D2H copy");
    delete scene;
    return 0;
}
