// pt_api.hip -- MI355X (gfx950 / CDNA4) path-tracing hot path + its C ABI (include/pt_amd.h).
//
// One iteration = `traceDepth` launches of ONE fused persistent kernel per bounce (the first builds its camera rays in
// registers): nearest-hit over the scene (geometry through the scalar path, materials in LDS) -> shade/scatter -> park
// emitter radiance -> stream compaction of the survivors straight into the next bounce's SoA path pool (wave64
// ballot/mbcnt ranks, LDS wave totals = workgroup-level exclusive scan per class; the tile's output runs are reserved
// with ONE atomic instruction on sharded position counters, chunks of the pool are handed out on demand).  No host
// round trip inside an iteration: live counts stay on the device.  The multi-workgroup ORDERED scan (two-level decoupled
// look-back) is the stream-compaction library in pt_compaction.h (pt_scan_exclusive_i32 / pt_compact_nonzero_i32).
// Files: pt_device.h (math), pt_trace.h (render kernels), pt_compaction.h, pt_test_kernels.h (primitives for the parity
// tests), this file (host side + C ABI).
//
// Replaces the unsolved pipeline of reference src/pathtrace.cu:133-167 (spec: SURVEY.md 3.4 S0-S9).
// HBM layout, kernels, rooflines: DESIGN.md.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <mutex>

#include "../../include/pt_amd.h"
#include "pt_compaction.h"
#include "pt_trace.h"
#include "pt_mesh_walk.h"
#include "pt_mesh.h"
#include "pt_denoise.h"
#include "pt_noise.h"
#include "pt_temporal.h"
#include "pt_spatial_var.h"
#include "pt_albedo.h"
#include "pt_camera_faces.h"
// The entry points of include/pt_amd_test.h (device primitives one by one, soundness sweeps, the fault-word hook) exist only in
// the second link target of this source, libpt_amd_test.so (-DPT_TEST_API): the product library exports none of them.
#ifdef PT_TEST_API
#include "../../include/pt_amd_test.h"
#include "pt_test_kernels.h"
#endif

using namespace ptd;
using namespace ptk;

static_assert(sizeof(PtGeom) == 236 && sizeof(PtMaterial) == 44 && sizeof(PtCamera) == 52,
              "layout must equal reference src/sceneStructs.h:18-47");
static_assert(sizeof(PtBumpBinding) == 24, "PtBumpBinding: 24 bytes (include/pt_amd.h)");
static_assert(sizeof(PtDenoiseParams) == 20, "PtDenoiseParams: 20 bytes (include/pt_amd.h)");
static_assert(sizeof(PtDenoiseVarParams) == 20, "PtDenoiseVarParams: 20 bytes (include/pt_amd.h)");
static_assert(sizeof(PtNoiseStats) == 40 && sizeof(PtNoiseTarget) == 28, "PtNoiseStats: 40 bytes, PtNoiseTarget: 28 (include/pt_amd.h)");
static_assert(PT_NOISE_TILE == ptk::kNoiseTile, "include/pt_amd.h and csrc/pt_noise.h name one tile size");
namespace {

// =====================================================================================================
// host side
// =====================================================================================================
thread_local std::string g_err = "";     // pt_last_error(): the calling thread's last failure

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHECK(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(PT_ERR_HIP, "HIP error (%s:%d): %s: %s", "pt_api.hip", __LINE__, #expr, \
                        hipGetErrorString(e_));                                                     \
    } while (0)
// ... and for the functions of this file that return PT_OK or what fail() returned
#define PTCHECK(expr)                                                                               \
    do {                                                                                            \
        int rc_ = (expr);                                                                           \
        if (rc_) return rc_;                                                                        \
    } while (0)

// an environment variable that switches something on (experiments and tests): set, and not to 0
bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && atoi(e);
}

#include "pt_owned.h"      // DevBuf, Stream, Event, HostBuf: the owners of everything this file holds on the device side, and the rule for process exit
#include "pt_host_scene.h"
#include "pt_scene_plan.h"

// One in-flight iteration: its own stream, path buffers, counters and deferred-radiance buffer.
struct Slot {
    Stream stream;
    DevBuf<float> pathbuf[2];      // two path pools (ping-pong by bounce), poolChunks * kChunk paths per array
    DevBuf<unsigned long long> chunkList[2];   // per pool: [kSeg][poolChunks] chunk lists of the queue it holds
    uint32_t gen[2] = {0, 0};      // per pool: serial number of the launch that filled it (tags the chunk-list entries)
    DevBuf<Ctrl> ctrl;
    DevBuf<float> contrib;         // maxBatch x W*H*3: an entry is valid while its bit of `hitMask` is set
    DevBuf<uint32_t> hitMask;      // ceil(maxBatch / 32) x W*H: which iterations of the batch wrote a pixel's `contrib`, zero between batches
    DevBuf<unsigned long long> meshHit;   // scenes with meshes: the walks' result per path of the bounce being launched (BounceArgs::meshHit)
    Event evDone;                      // all bounce launches of the slot's current iteration finished
    Event evCommitted;                 // k_commit consumed `contrib` (cleared the masks' bits)
    int parity = 0;                // which half of Ctrl::cursor the slot's next batch uses
};

// PT_FLAG_TEMPORAL: what a context keeps of the view its last renderer rendered (pt_temporal.h).  Made by pt_init over a live renderer
// (capture_history), read by denoise_var_run, dropped by free_renderer unless pt_init asks to keep it.
struct History {
    DevBuf<float4> hc[2];           // (mean r, g, b, mean squared luminance): a ping-pong pair, `cur` the half that holds the history ...
    DevBuf<float> hn[2];            // ... and the effective sample counts, 0 = none
    DevBuf<float4> ha[2];           // PT_FLAG_DEMOD_HISTORY: ... and (the mean first-hit albedo, unfloored; the uncapped count), the same ping-pong
    DevBuf<float4> hpos, hnrm;      // the old view's guide buffers of guide_iter 1, handed over by its renderer
    TemporalCam cam = {};           // the old view's camera
    int cur = 0, W = 0, H = 0;
    bool live = false;
    bool albedo = false;            // the renderer that made it carried PT_FLAG_DEMOD_HISTORY: ha[cur] is live too
    // PT_FLAG_OBJECT_HISTORY: the geoms of the view the history was captured from -- the poses it is in --, and, while the renderer that
    // reads it shows a primitive in another pose, the motion table (pt_temporal.h, MOTION) with its host copy and the cap that goes with it
    std::vector<PtGeom> pose;
    DevBuf<float4> motion;          // MotionRow per primitive; none: every primitive unmoved -- PT_FLAG_TEMPORAL's launches
    std::vector<MotionRow> motionHost;
    float cap = PT_TEMPORAL_MAX_HISTORY;
};

// How a scene table differs from the plain one -- a buffer where the plan's vector is not empty, of its size, refreshed by a camera move
// whose plan holds other bytes.
struct TableRule {
    bool evenEmpty = false;         // a buffer even for an empty table: a kernel may be handed its pointer
    size_t slack = 0;               // elements allocated behind the table's, left uninitialised
    bool cameraInvariant = false;   // no camera changes it: pt_init uploads it and drops the host's copy, a move compares its size alone
    // the elements pt_init allocates for a table of n (DevBuf::upload)
    size_t allocated(size_t n) const { return n || evenEmpty ? std::max<size_t>(n + slack, 1) : 0; }
};

// The scene's tables on the device, each as the plan made it (ScenePlan).  A table is named three times in this file: its buffer here, its
// line in for_each -- the plan's vector it comes from and its rule -- and its pointer in fill(); pt_init and the camera move are actions
// handed to for_each.
struct SceneTables {
    DevBuf<GeomDev> dgeoms;
    DevBuf<unsigned char> dGeomHit; // GeomHitDev[ngeoms], as the kernels stage it in LDS (scenes that are not sphere-heavy; those: one image of their tables)
    DevBuf<float> dRows;            // sphere-heavy scenes of hundreds of primitives: the matrix rows that do not go to LDS (BounceArgs::rows)
    DevBuf<MaterialDev> dmats;
    DevBuf<WallBox> dwalls;
    DevBuf<SphereCull> dSphCull;    // sphere-heavy scenes: packed culling data of the spheres, and ...
    DevBuf<SphereCull> dSphGroups;  // ... scenes of hundreds of them: the bounding balls of the table's groups (BounceArgs::sphGroups)
    DevBuf<int> dCamWave, dCamSigIdx;   // camera rays: the packed work list (build_camera_list), or none
    DevBuf<int> dCamFace;               // ... and its waves' resolved cube faces (CameraList::face)
    DevBuf<uint32_t> dCamPix;
    DevBuf<int> dRowOff, dRowIdx;   // camera-ray bounce: per image row, the primitives whose pixel rectangle covers it
    DevBuf<int> dClassIdx;          // later bounces: per queue class, the primitives to look at (KParams::classOff)
    DevBuf<ptd::MeshUnit> dMeshRecs;   // ptd::MeshUnit[]: triangles and inner nodes of every mesh of the scene (k_bounce<., ., ., true>)
    // textured scenes (k_bounce<..., TEX>): BounceArgs::texGeom / texDesc / texels / texUV
    DevBuf<ptd::TexGeom> dTexGeom;
    DevBuf<int4> dTexDesc;
    DevBuf<float4> dTexels, dTexUV;
    // bump-mapped scenes (k_bounce<..., BUMP>): BounceArgs::bumpGeom / bumpUV / bumpTan
    DevBuf<ptd::BumpGeom> dBumpGeom;
    DevBuf<float4> dBumpUV, dBumpTan;
    // scenes with meshes, whose walks run ahead of every bounce launch (k_mesh_walk): the meshes alone per queue class / in all / per image row
    DevBuf<int> dWalkIdx, dWalkRowOff;
    DevBuf<WalkMesh> dWalkMeshRows;    // ptk::WalkMesh per mesh (BounceArgs::walkMeshRows)

    // f(buffer, the held plan's vector -- nullptr without a held plan --, the new plan's vector, the table's rule) for every table, in
    // pt_init's order of uploads; stops at the first f that does not answer PT_OK.  mesh, grouped: the new plan's (a scene without
    // meshes has no walks' tables at all, an ungrouped one no groups' table).
    template <class F>
    int for_each(const ScenePlan *held, ScenePlan &now, bool mesh, bool grouped, F &&f) {
        const ScenePlan &h = held ? *held : now;
        const auto of = [held](const auto &v) { return held ? &v : nullptr; };
        const TableRule plain{}, evenEmpty{true}, invariant{false, 0, true};
        PTCHECK(f(dgeoms, of(h.hg), now.hg, plain));
        PTCHECK(f(dmats, of(h.hm), now.hm, plain));
        PTCHECK(f(dGeomHit, of(h.geomHit), now.geomHit, plain));
        PTCHECK(f(dRows, of(h.rowsGlobal), now.rowsGlobal, plain));
        PTCHECK(f(dwalls, of(h.hw), now.hw, plain));
        PTCHECK(f(dTexGeom, of(h.texGeom), now.texGeom, plain));
        PTCHECK(f(dTexDesc, of(h.texDesc), now.texDesc, plain));
        PTCHECK(f(dTexels, of(h.texels), now.texels, invariant));
        PTCHECK(f(dTexUV, of(h.texUV), now.texUV, plain));
        PTCHECK(f(dBumpGeom, of(h.bumpGeom), now.bumpGeom, plain));
        PTCHECK(f(dBumpUV, of(h.bumpUV), now.bumpUV, plain));
        PTCHECK(f(dBumpTan, of(h.bumpTan), now.bumpTan, plain));
        if (mesh) {
            PTCHECK(f(dMeshRecs, of(h.meshRecs), now.meshRecs, TableRule{true, 4, true}));     // (+ 4: a walk may read the record behind the last one)
            PTCHECK(f(dWalkIdx, of(h.walkIdx), now.walkIdx, evenEmpty));
            PTCHECK(f(dWalkMeshRows, of(h.walkMeshRows), now.walkMeshRows, evenEmpty));
        }
        PTCHECK(f(dSphCull, of(h.sc), now.sc, plain));
        if (grouped) PTCHECK(f(dSphGroups, of(h.groups), now.groups, evenEmpty));
        PTCHECK(f(dRowOff, of(h.cc.rowOff), now.cc.rowOff, plain));
        PTCHECK(f(dRowIdx, of(h.cc.rowIdx), now.cc.rowIdx, plain));
        PTCHECK(f(dCamPix, of(h.cl.pix), now.cl.pix, plain));
        PTCHECK(f(dCamWave, of(h.cl.wave), now.cl.wave, plain));
        PTCHECK(f(dCamSigIdx, of(h.cl.sigIdx), now.cl.sigIdx, plain));
        PTCHECK(f(dCamFace, of(h.cl.face), now.cl.face, plain));
        PTCHECK(f(dWalkRowOff, of(h.walkRowOff), now.walkRowOff, plain));
        PTCHECK(f(dClassIdx, of(h.classIdx), now.classIdx, plain));
        return PT_OK;
    }

    // a launch's pointers to the tables (a table the scene does not have: null, and its kernels do not ask)
    void fill(BounceArgs &ba) const {
        ba.ggeoms = dgeoms.p; ba.gmats = dmats.p; ba.ghit = reinterpret_cast<const float4 *>(dGeomHit.p);
        ba.sphCull = dSphCull.p; ba.classIdx = dClassIdx.p;
        ba.rowOff = dRowOff.p; ba.rowIdx = dRowIdx.p;
        ba.camPix = dCamPix.p; ba.camWave = dCamWave.p; ba.camSigIdx = dCamSigIdx.p; ba.camFace = dCamFace.p;
        ba.walls = dwalls.p;
        ba.meshRecs = reinterpret_cast<const float4 *>(dMeshRecs.p);
        ba.rows = reinterpret_cast<const float4 *>(dRows.p);
        ba.walkIdx = dWalkIdx.p; ba.walkRowOff = dWalkRowOff.p;
        ba.walkMeshRows = reinterpret_cast<const float4 *>(dWalkMeshRows.p);
        ba.sphGroups = dSphGroups.p;
        ba.texGeom = dTexGeom.p; ba.texDesc = dTexDesc.p; ba.texels = dTexels.p; ba.texUV = dTexUV.p;
        ba.bumpGeom = dBumpGeom.p; ba.bumpUV = dBumpUV.p; ba.bumpTan = dBumpTan.p;
    }
};

// PT_FLAG_MOTION: one planned pose of the scene -- everything a launch reads that the pose decides: the plan's scalars, the tables (but
// the ones no pose changes, texels and mesh records, which stay in State::tab: held once), the forms of k_bounce and the grids.  The
// pose the renderer is in lives in State's own members; the others wait here, and activate_step exchanges the two on the host.
struct Pose {
    PlanScalars scalars;
    SceneTables tab;
    const void *kernFirst = nullptr, *kernNext = nullptr;
    int gridWalk = 0, gridWalkFirst = 0, grid = 0, gridFirst = 0;
};

// (it keeps the scalars of the scene's plan -- cam, prm, P, nLocal, flags, the flags that pick the forms of k_bounce, the sizes -- as its base)
struct State : PlanScalars {
    bool init = false;
    int device = 0;
    hipStream_t stream = nullptr;   // the caller's stream, borrowed: commits, PBO conversion, readback
    float *image = nullptr;         // the accumulator the kernels add to: the caller's (PtOptions::accum_dev, never freed here), or ...
    DevBuf<float> imageOwn;         // ... the renderer's own
    DevBuf<float> moments;          // PT_FLAG_MOMENTS: per pixel the sum of its samples' squared luminance (k_commit<true>); always the renderer's own
    Slot slot[kMaxSlots];
    SceneTables tab;                // the scene's tables
    // the denoiser (pt_denoise.h), all allocated on first use: the guide buffers of iteration dnGuideIter (0: none yet), the float4 images
    // the filter's levels pass on, and the packed RGB the last level writes.  (PT_FLAG_DISPLAY_FILTER: pt_init allocates the four float4
    // images and dnRgba -- what the display path touches -- so that pt_iterate allocates nothing.)
    DevBuf<float4> dnPosT, dnNrmId, dnPing[2];
    DevBuf<float> dnOut;
    DevBuf<uchar4> dnRgba;          // pt_denoise_rgba8's bytes, and pt_readback_rgba8's under PT_FLAG_DISPLAY_FILTER
    DevBuf<float> dnVar;            // pt_variance's / pt_denoise_var's variance image
    DevBuf<float> dnCount;          // PT_FLAG_SPATIAL_VARIANCE: the effective sample counts of a one-sample frame (pt_spatial_var.h); pt_init's
    DevBuf<float4> albedo;          // PT_FLAG_DEMODULATE: per pixel (the sum of the committed iterations' first-hit albedo, their number) (pt_albedo.h); pt_init's
    DevBuf<float4> dnAlbedo;        // PT_FLAG_DEMOD_HISTORY: (Ab, tot), the blend of the reprojected albedo with `albedo` (pt_temporal.h, ALBEDO); pt_init's
    int dnGuideIter = 0;
    // the noise statistics (pt_noise.h), all allocated on first use: the frame's two result words on the device, the tile map, and -- for
    // pt_iterate_until, whose checks the host reads while the stream runs on -- two copies of the words in page-locked memory, each with the
    // event that says its copy has landed
    DevBuf<uint32_t> noiseFrame;
    DevBuf<float> noiseMap;
    HostBuf<uint32_t> noiseHost;        // 2 x 2 words
    Event noiseEv[2];
    int gridWalk = 0, gridWalkFirst = 0;      // the grids of the meshes' walks (k_mesh_walk) ...
    int grid = 0;           // ... the persistent grid of k_bounce<false>
    int gridFirst = 0;      // ... and of k_bounce<true> (its own register budget, hence its own residency)
    const void *kernFirst = nullptr, *kernNext = nullptr;   // the forms of k_bounce the camera-ray launch / the later ones take (bounce_form)
    // PT_FLAG_MOTION: the PT_MOTION_STEPS poses (none without the flag); poses[step] is the slot of the one the members above hold now
    std::vector<Pose> poses;
    int step = 0;
    // what pt_init allocated of scene tables (pt_test_pose_tables): the buffers and bytes of ONE pose's own tables (step 0's), of the
    // tables held once whatever the number of poses (the camera-invariant ones), and the bytes of every pose's own tables together
    struct TableCount { long long ownBuffers = 0, ownBytes = 0, sharedBuffers = 0, sharedBytes = 0, allOwnBytes = 0; } tables;
    long long iterations = 0;
    long long committed = 0; // iterations committed into the accumulators since pt_init: `iterations` without pt_counters_reset's zeroing (the capture's n)
    long long seq = 0;      // batches enqueued since pt_init: slot = seq % nslots
    // PT_FLAG_TRACE_AHEAD: batches traced ahead of the pt_iterate calls that will ask for their iterations, oldest first.
    // A parked batch occupies its slot (radiance buffers, iteration masks) until its last iteration is committed or it
    // is discarded; the parked slots are the `ahead.size()` slots before seq % nslots in the rotation.
    struct Parked { int slot, first, count, next; bool waited; };   // iterations first .. first + count - 1, the next one to commit = first + next;
                                                                    // waited: the caller's stream already waits for the batch's launches
    std::deque<Parked> ahead;
    uint32_t launchSerial = 0;   // bounce launches since pt_init
    // host buffer of pt_readback, page-locked on first use so the per-iteration D2H copy of the reference protocol
    // (src/pathtrace.cu:170-171) runs at PCIe rate instead of through a pageable staging copy
    void *pinnedHost = nullptr;     // the caller's memory, borrowed: registered and unregistered by hand (pt_owned.h: the rule for process exit)
    size_t pinnedBytes = 0;
    // kernel timing
    std::vector<Event> evBounce;      // the timed launches not yet resolved: each one's start and end, in pairs
    std::vector<Event> evFree;        // resolved timing events, reused (creating two per launch cost 1 % of a timed step)
    double msBounce = 0;
    long long nBounce = 0;
    // The sticky fault word once more, in page-locked HOST memory the kernels can write (a fault path stores it there too): pt_readback
    // and pt_readback_rgba8, which synchronise anyway, then report a faulted render without a device-to-host copy of their own.
    HostBuf<uint32_t> hostFault;         // host address
    uint32_t *hostFaultDev = nullptr;    // the same word as the kernels address it (derived from hostFault, not owned)
    // device groups (pt_group.h): the full frame the NEXT commit also copies this shard's pixels into (k_commit's `snap`: the snapshot a
    // frame reduce reads), and the event -- the reduce that last read that buffer -- the commit has to wait for first.  Set per call.
    float *snapTarget = nullptr;    // the group's, borrowed
    hipEvent_t snapWait = nullptr;  // the group's, borrowed
    // what the pt_set_* calls last registered, consumed by the next pt_init (kept across pt_free: the reference's Free -> Init restart
    // protocol re-initialises the same scene), and what was registered when the renderer was initialised: the scene its camera moves
    // plan, whatever has been registered since
    Registered reg, initReg;
    // ... and, across a pt_init over the live renderer only, the last view's samples (PT_FLAG_TEMPORAL)
    History hist;
    // the camera move: what the renderer was initialised with -- pt_init's scene arguments and effective options (a few hundred bytes per
    // primitive) -- and the plan it holds: the tables as the device has them (but the camera-invariant ones, whose buffers say their
    // sizes), so that a move uploads only the tables whose bytes differ
    std::vector<PtGeom> inGeoms;
    std::vector<PtMaterial> inMats;
    int inDepth = 0;
    PtOptions inOpts = {};
    std::unique_ptr<ScenePlan> held;
    // ... and what its certificates on the device need (k_camera_faces), made by the first move: a stream of their own -- the renderer's may
    // hold a frame's work -- and the pixel words and face bytes of one move
    Stream camStream;
    DevBuf<uint32_t> camPixScratch;
    DevBuf<signed char> camFaceScratch;
    // Nothing to drain or release (the history aside): no pt_init has come as far as its device half since the last free -- it begins by taking the
    // plan's scalars, nslots >= 1 among them, before its first allocation -- and no host buffer is registered.  Answered without a HIP call.
    bool holds_nothing() const { return nslots == 0 && !pinnedHost; }
};

// Renderer instances.  The reference keeps its renderer in file-static globals (src/pathtrace.cu:70-71: one per process, not
// re-entrant); so did rounds 1-4 here.  Now a renderer is a CONTEXT: the C ABI's functions act on the calling thread's CURRENT
// context -- the process-wide default one unless pt_ctx_make_current named another (include/pt_amd.h) -- so that one host process
// drives several renderers: one per device of a node (row shards of one frame, pt_group_*), or several on one device.
State g_default;
thread_local State *t_ctx = &g_default;
inline State &R() { return *t_ctx; }
std::mutex g_ctxMutex;                    // guards g_contexts
std::vector<State *> g_contexts;          // every context pt_ctx_create made and pt_ctx_destroy has not released (the exit handler frees their renderers)
std::mutex g_groupMutex;                  // guards g_groups
std::vector<PtGroup *> g_groups;          // every group pt_group_create made and pt_group_destroy has not released (the exit handler destroys them:
                                          // their issuing threads, communicators, streams and frame buffers -- pt_group.h)

// PT_FLAG_MOTION: the renderer's pose against a waiting one -- a host-side exchange of the members a launch reads.  Launches take
// pointers by value and no table is ever rewritten, so batches of different poses may be in flight on neighbouring slots: no drain.
void exchange_pose(State &S, Pose &p) {
    std::swap(static_cast<PlanScalars &>(S), p.scalars);
    std::swap(S.tab, p.tab);
    std::swap(S.tab.dTexels, p.tab.dTexels);        // (held once: they stay where they are)
    std::swap(S.tab.dMeshRecs, p.tab.dMeshRecs);
    std::swap(S.kernFirst, p.kernFirst); std::swap(S.kernNext, p.kernNext);
    std::swap(S.gridWalk, p.gridWalk); std::swap(S.gridWalkFirst, p.gridWalkFirst);
    std::swap(S.grid, p.grid); std::swap(S.gridFirst, p.gridFirst);
}
void activate_step(State &S, int step) {
    if (S.poses.empty() || step == S.step) return;
    exchange_pose(S, S.poses[(size_t)S.step]);
    exchange_pose(S, S.poses[(size_t)step]);
    S.step = step;
}
// the step iteration `iter` renders, and the first iteration behind its run (include/pt_amd.h, "motion blur")
inline int motion_step(int iter) { return PT_MOTION_STEP(iter); }
inline int motion_run_end(int iter) { return ((iter - 1) / PT_MOTION_RUN + 1) * PT_MOTION_RUN + 1; }

int count_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int reset_ctrl(Ctrl *dev, hipStream_t st) {
    HIPCHECK(hipMemsetAsync(dev, 0, sizeof(Ctrl), st));
    HIPCHECK(hipStreamSynchronize(st));
    return PT_OK;
}

PathPool pool(const Slot &sl, int which) {
    PathPool p;
    p.base = sl.pathbuf[which].p;
    p.list = sl.chunkList[which].p;
    p.cap = (uint32_t)R().poolChunks << R().prm.chunkShift;
    return p;
}

void recycle_events(std::vector<Event> &v) {      // the timing events of `v` back into the pool
    for (Event &e : v) R().evFree.push_back(std::move(e));
    v.clear();
}

int resolve_events(std::vector<Event> &v, double &ms, long long &n) {
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
        float t = 0;
        HIPCHECK(hipEventSynchronize(v[i + 1]));
        HIPCHECK(hipEventElapsedTime(&t, v[i], v[i + 1]));
        ms += t;
        n += 1;
    }
    recycle_events(v);
    return PT_OK;
}

// The forms of k_bounce.  A form is the word of its nine template flags, in the template's order: FIRST (camera rays), MANY (per-lane
// lists of the swept primitives: scenes with more than kBinMax of them), DOF (thin lens: the camera-ray launch only), MESH (scenes with
// triangle meshes), PLAIN, CUBES, GROUPS, TEX, BUMP.
enum : uint32_t { kbFirst = 1, kbMany = 2, kbDof = 4, kbMesh = 8, kbPlain = 16, kbCubes = 32, kbGroups = 64, kbTex = 128, kbBump = 256, kbForms = 512 };

// The forms that are instantiated -- each is a large kernel, so these 48 of the 512 words and no other: the textured ones (24: with and
// without BUMP, never PLAIN or GROUPS, MANY always in the form that sweeps cubes too), the two PLAIN ones, the four GROUPS ones, and the
// 18 of MANY (with or without CUBES) x MESH x camera rays with a lens / without / later bounces.
constexpr bool bounce_form_valid(uint32_t f) {
    const bool F = f & kbFirst, M = f & kbMany, D = f & kbDof, ME = f & kbMesh, PL = f & kbPlain, CU = f & kbCubes, GR = f & kbGroups,
               TX = f & kbTex, BU = f & kbBump;
    return f < kbForms && (!D || F) && (!BU || TX) && (!CU || M) && (!TX || (!PL && !GR && CU == M)) && (!PL || (!M && !ME && !D && !GR)) &&
           (!GR || (M && !ME && !D));
}
template <uint32_t f>
const void *kb() {
    if constexpr (bounce_form_valid(f))
        return reinterpret_cast<const void *>(k_bounce<(f & kbFirst) != 0, (f & kbMany) != 0, (f & kbDof) != 0, (f & kbMesh) != 0, (f & kbPlain) != 0,
                                                       (f & kbCubes) != 0, (f & kbGroups) != 0, (f & kbTex) != 0, (f & kbBump) != 0>);
    else
        return nullptr;
}
template <size_t... f>
const void *bounce_kernel_of(uint32_t form, std::index_sequence<f...>) {
    static const void *const table[] = {kb<(uint32_t)f>()...};
    return form < kbForms ? table[form] : nullptr;
}
// the kernel of a form, or nullptr: not one of the 48
const void *bounce_kernel(uint32_t form) { return bounce_kernel_of(form, std::make_index_sequence<kbForms>()); }

// The form a launch takes: `first` is the launch's (the camera-ray bounce), the rest the renderer's state (PlanScalars: dof, many, sweptCubes,
// mesh, grouped, tex, bump, plain).
uint32_t bounce_form(bool first, bool dof, bool many, bool sweptCubes, bool mesh, bool grouped, bool tex, bool bump, bool plain) {
    const bool D = first && dof;                      // thin lens: the camera-ray launch only
    uint32_t f = (first ? kbFirst : 0u) | (many ? kbMany : 0u) | (D ? kbDof : 0u) | (mesh ? kbMesh : 0u);
    // textured scenes: forms of their own -- never PLAIN or GROUPS (textured scenes are never grouped: the grouped sweep is the ungrouped
    // one's result, bit for bit, and the TEX forms leave it out), and MANY always in the form that sweeps cubes too
    if (tex) f |= kbTex;
    if (bump) f |= kbBump;                            // bump-mapped scenes: the TEX forms again, with BUMP
    // plain scenes -- diffuse / emissive / perfect-mirror materials, no README extra: the instantiations without the rarer branches
    if (!tex && plain && !mesh && !many && !D) f |= kbPlain;
    // many small primitives, cubes among them: the per-lane tests take either type
    if (many && (tex || sweptCubes)) f |= kbCubes;
    // hundreds of swept primitives: the two-level sweep, nothing of the scene's tables in LDS -- the later bounces and the (pinhole)
    // camera-ray bounce, whose hit records, frames and rows come from global memory too; the grouped camera-ray bounce with a lens falls
    // back to the flat sweep
    if (!tex && grouped && !D) f |= kbGroups;
    return f;
}
// ... resolved once by pt_init (State::kernFirst / kernNext); a state whose form is not instantiated is an internal error, never a fallback
int resolve_bounce_kernel(const PlanScalars &s, bool first, const void **kernel) {
    const uint32_t f = bounce_form(first, s.dof, s.many, s.sweptCubes, s.mesh, s.grouped, s.tex, s.bump, s.plain);
    *kernel = bounce_kernel(f);
    if (!*kernel)
        return fail(PT_ERR_INVALID, "pt_init: internal error: no k_bounce form 0x%x (FIRST %d MANY %d DOF %d MESH %d PLAIN %d CUBES %d GROUPS %d TEX %d BUMP %d)", f,
                    !!(f & kbFirst), !!(f & kbMany), !!(f & kbDof), !!(f & kbMesh), !!(f & kbPlain), !!(f & kbCubes), !!(f & kbGroups), !!(f & kbTex), !!(f & kbBump));
    return PT_OK;
}

const void *walk_kernel(bool first, bool dof) {
    if (R().walkMeshLds != 0) {      // the meshes' rows in LDS (scenes of at most kWalkMeshLdsMax meshes)
        if (first) return dof ? reinterpret_cast<const void *>(k_mesh_walk<true, true, true>) : reinterpret_cast<const void *>(k_mesh_walk<true, false, true>);
        return reinterpret_cast<const void *>(k_mesh_walk<false, false, true>);
    }
    if (first) return dof ? reinterpret_cast<const void *>(k_mesh_walk<true, true, false>) : reinterpret_cast<const void *>(k_mesh_walk<true, false, false>);
    return reinterpret_cast<const void *>(k_mesh_walk<false, false, false>);
}

int launch_bounce(Slot &sl, int iter, int batch, int depth, bool lastBounce, float *contrib, bool nextIsLast = false) {
    const PathPool in = pool(sl, (depth - 1) & 1);
    const PathPool out = pool(sl, depth & 1);
    // chunk-list entries carry the serial number of the launch that wrote them (never 0)
    const uint32_t genIn = sl.gen[(depth - 1) & 1];
    if (++R().launchSerial == 0u) ++R().launchSerial;
    const uint32_t genOut = sl.gen[depth & 1] = R().launchSerial;
    Event e0, e1;
    if (R().flags & PT_FLAG_KERNEL_TIMING) {
        for (Event *e : {&e0, &e1}) {
            if (!R().evFree.empty()) { *e = std::move(R().evFree.back()); R().evFree.pop_back(); }
            else PTCHECK(e->create(hipEventDefault));
        }
        HIPCHECK(hipEventRecord(e0, sl.stream));
    }
    BounceArgs ba;
    ba.prm = R().prm;
    ba.iter = iter; ba.batch = batch; ba.depth = depth; ba.lastBounce = lastBounce ? 1 : 0; ba.parity = sl.parity;
    ba.histShift = R().prm.histBits * (depth - 1);
    ba.genIn = genIn; ba.genOut = genOut;
    ba.in = in; ba.out = out;
    ba.tile.inBase = in.base; ba.tile.inList = in.list; ba.tile.inCap = in.cap;
    ba.tile.genIn = genIn; ba.tile.poolChunks = (uint32_t)R().prm.poolChunks; ba.tile.chunkShift = (uint32_t)R().prm.chunkShift;
    ba.tile.skipNonCandidates = (lastBounce && R().prm.emittersBinned) ? 1u : 0u;
    ba.tile.hot = (lastBounce ? kHotLast : 0u) | (R().prm.allClassified ? kHotAllClassified : 0u) | (contrib ? kHotContrib : 0u) |
                  ((R().prm.directDepth != 0 && depth == R().prm.directDepth && R().prm.nEmit > 0) ? kHotToLight : 0u) |
                  (R().prm.contribLocal ? kHotContribLocal : 0u) | ((R().flags & PT_FLAG_MIXTURE_WEIGHTED) ? kHotMixWeighted : 0u) | ((uint32_t)R().prm.nWalls << 8) | ((uint32_t)R().prm.nSlotWalls << 11) | ((uint32_t)R().prm.nPlaneWalls << 17) |
                  ((uint32_t)R().prm.nBinned << 14) | ((uint32_t)R().prm.nmats << 20);
    // sphere clusters: the queue that ENTERS the last bounce carries other candidate bits (k_bounce: kHotWritesLastBits) -- that launch only asks
    // whether a path ends on an emitter, and with every emitter binned it visits the tiles of the binned primitives' candidates alone
    const bool lastBits = R().many && !R().mesh && R().prm.sphOMax > 0.0f && R().prm.emittersBinned;
    if (lastBits && nextIsLast) ba.tile.hot |= kHotWritesLastBits;
    if (lastBits && lastBounce && depth > 1) ba.tile.hot |= kHotReadsLastBits;
    ba.ctrl = sl.ctrl.p; ba.contrib = contrib; ba.hitMask = sl.hitMask.p; ba.meshHit = sl.meshHit.p;
    ba.hostFault = R().hostFaultDev;
    R().tab.fill(ba);
    memcpy(ba.walkClassOff, R().walkClassOff, sizeof ba.walkClassOff);
    ba.walkAll0 = R().walkAll0; ba.walkAll1 = R().walkAll1;
    ba.walkMeshLds = R().walkMeshLds;
    void *kargs[] = {&ba};
    const bool first = depth == 1;
    // scenes with meshes: the walks of this bounce's rays, ahead of it (pt_mesh_walk.h)
    if (R().mesh)
        HIPCHECK(hipLaunchKernel(walk_kernel(first, first && R().dof), dim3(first ? R().gridWalkFirst : R().gridWalk), dim3(kBlock), kargs, R().ldsWalk, sl.stream));
    HIPCHECK(hipLaunchKernel(first ? R().kernFirst : R().kernNext, dim3(first ? R().gridFirst : R().grid), dim3(kBlock), kargs, first ? R().ldsBytes : R().ldsBytesNext, sl.stream));
    if (e0) {
        HIPCHECK(hipEventRecord(e1, sl.stream));
        R().evBounce.push_back(std::move(e0));
        R().evBounce.push_back(std::move(e1));
        if (R().evBounce.size() > 2 * 8192) {
            int rc = resolve_events(R().evBounce, R().msBounce, R().nBounce);
            if (rc) return rc;
        }
    }
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

// scan library workspace: the chunk totals, one buffer per stream (calls on different streams may overlap; calls on one
// stream are ordered, so they share it)
struct ScanWs {
    int device = -1;                 // the device the buffers live on
    DevBuf<uint32_t> partial;        // [kScanChunksMax + 1]
    DevBuf<unsigned long long> chained;      // k_scan_chained: {ticket, sums[kScanChunksMax]}
    uint32_t gen = 0;                // calls of the chained scan on this stream (tags the sums; never 0)
};
std::map<std::pair<int, hipStream_t>, ScanWs> g_scan;   // per (device, stream): the NULL stream -- or an equal handle -- of another device is another workspace
std::mutex g_scanMutex;              // the scan library may be called from several host threads (one stream each)

// The caller HOLDS g_scanMutex from here until its launches that use the workspace are enqueued: pt_free, which releases the
// workspaces, takes the same lock first and then waits for the device -- so a workspace is never freed between its look-up and the
// kernels that use it (round 3 handed the pointer out of the lock: a second host thread could enqueue on freed memory).
int scan_ws(hipStream_t st, ScanWs **out) {
    int dev = 0;
    HIPCHECK(hipGetDevice(&dev));    // the device current at the call: where the caller's buffers live and the kernels will run
    ScanWs &W = g_scan[std::make_pair(dev, st)];          // (std::map: the reference stays valid while other streams are added)
    W.device = dev;
    if (!W.partial.p) PTCHECK(W.partial.alloc((size_t)kScanChunksMax + 1));
    if (!W.chained.p) PTCHECK(W.chained.alloc_zeroed((size_t)kScanChunksMax + 1));
    *out = &W;
    return PT_OK;
}
// releases every stream's workspace: the PUBLIC pt_free and the process's exit only -- not the pt_free inside pt_init (the
// reference's Free -> Init restart), which other host threads' scans must survive.  Under the lock: no scan call is between its
// look-up and its launches; then everything enqueued is waited for, then freed.
void scan_release() {
    std::lock_guard<std::mutex> lock(g_scanMutex);
    if (g_scan.empty()) return;
    int cur = -1, synced = -1;
    (void)hipGetDevice(&cur);
    for (auto &kv : g_scan) {        // (ordered by device: every device that owns a workspace is waited for once, then its buffers go)
        if (kv.second.device != synced) {
            (void)hipSetDevice(kv.second.device);
            (void)hipDeviceSynchronize();
            synced = kv.second.device;
        }
        kv.second.partial.release();
        kv.second.chained.release();
    }
    g_scan.clear();
    if (cur >= 0) (void)hipSetDevice(cur);
}
bool scan_in_use() {
    std::lock_guard<std::mutex> lock(g_scanMutex);
    return !g_scan.empty();
}
// the array as chunks of whole tiles: at most kScanChunksMax of them
void scan_chunks(long long n, long long *tilesPerChunk, int *chunks) {
    const long long tiles = (n + kScanTile - 1) / kScanTile;
    const long long per = (tiles + kScanChunksMax - 1) / kScanChunksMax;
    *tilesPerChunk = per < 1 ? 1 : per;
    *chunks = (int)((tiles + *tilesPerChunk - 1) / *tilesPerChunk);
}

// wait for every stream the renderer uses
int sync_all() {
    for (int i = 0; i < R().nslots; ++i) HIPCHECK(hipStreamSynchronize(R().slot[i].stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return PT_OK;
}

// what a set fault word (Ctrl::error) is reported as
std::string fault_message(uint32_t bits) {
    char buf[160];
    snprintf(buf, sizeof buf, "device fault 0x%x:%s%s (results of this render are void; re-init)", bits,
             (bits & kFaultPoolExhausted) ? " path pool exhausted" : "", (bits & kFaultReserveTimeout) ? " chunk reservation timed out" : "");
    return buf;
}

int check_device_fault() {
    int rc = sync_all();
    if (rc) return rc;
    for (int i = 0; i < R().nslots; ++i) {
        uint32_t err = 0;
        HIPCHECK(hipMemcpy(&err, &R().slot[i].ctrl.p->error, sizeof err, hipMemcpyDeviceToHost));
        if (err) return fail(PT_ERR_DEVICE, "%s", fault_message(err).c_str());
    }
    return PT_OK;
}

// pt_readback / pt_readback_rgba8 have just synchronised the caller's stream: every launch whose radiance the image holds has
// finished, and a fault any of them raised is in the host-visible copy of the fault word -- no device-to-host copy on the
// good path.  A faulted render is then reported like pt_sync does (the image has been copied all the same; it is void).
int readback_fault() {
    if (R().hostFault && *(volatile uint32_t *)R().hostFault != 0u) {
        int rc = check_device_fault();
        if (rc) return rc;
        return fail(PT_ERR_DEVICE, "device fault (results of this render are void; re-init)");
    }
    return PT_OK;
}

// The grid of a persistent kernel: the workgroups of it a CU holds at once x the CUs -- for k_bounce, or for the mesh walk ahead of it
int persistent_grid(const void *kernel, size_t lds, bool walk, int *grid) {
    int dev = 0;
    HIPCHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, dev));
    int perCU = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kBlock, lds));
    if (perCU < 1) perCU = 1;
    if (walk) {      // (every workgroup that fits: none of the bounce kernel's caps)
        if (const char *e = getenv("PT_AMD_WALK_BLOCKS_PER_CU")) perCU = std::max(1, atoi(e));   // experiments only
    } else {
        // All four instantiations fit eight workgroups per CU (<= 80 SGPRs, <= 64 VGPRs; the sphere-list variants seven).  A
        // launch that has the GPU to itself (pipeline_depth 1) is fastest with all of them (0.253 ms against 0.274 with six);
        // with batches in flight on neighbouring streams six per launch is better (131.2 G paths/s against 128.9 with eight):
        // the two free wave slots per SIMD go to the neighbouring batch's launches, which fill this launch's tail.
        int cap = R().nslots > 1 ? 6 : 8;
        // PT_FLAG_TRACE_AHEAD (one call and one small commit per iteration while batches are traced ahead): four, so that the commit -- and the
        // copies and collectives a caller puts behind it every iteration -- find free wave slots next to two batches' persistent workgroups
        // instead of waiting for one of them to end (config C3 as written: 0.0538 -> 0.0492 ms per iteration, profiles/r05_c3_experiments.txt)
        if ((R().flags & PT_FLAG_TRACE_AHEAD) && R().nslots > 1) cap = 4;
        if (const char *e = getenv("PT_AMD_BLOCKS_PER_CU")) cap = atoi(e);   // experiments only
        if (perCU > cap) perCU = cap;
    }
    *grid = prop.multiProcessorCount * perCU;
    if (const char *e = getenv("PT_AMD_MAX_GRID")) *grid = std::max(1, std::min(*grid, atoi(e)));   // tests: a small or partitioned device's grid
    return PT_OK;
}

constexpr int kIterEnd = 1 << 22;     // iterations are 1 .. kIterEnd - 1 (seed bits, pathtrace.cu:43)

// the bounce launches of iterations first_iter .. first_iter + count - 1 as one wavefront batch on the slot's stream; the
// radiance they find is parked in the slot's buffers until a commit consumes it
int trace_batch(Slot &sl, int first_iter, int count) {
    // the slot's radiance buffers must have been consumed by the commit of its previous batch
    HIPCHECK(hipStreamWaitEvent(sl.stream, sl.evCommitted, 0));
    const int D = R().prm.traceDepth;
    for (int d = 1; d <= D; ++d) {
        int rc = launch_bounce(sl, first_iter, count, d, d == D, sl.contrib.p, d + 1 == D);
        if (rc) {
            // a launch failed with part of the batch enqueued: counters, parity and radiance buffers are half-updated, so the
            // renderer refuses further work until it is re-initialised (pt_free still releases everything)
            if (d > 1) R().init = false;
            return rc;
        }
    }
    sl.parity ^= 1;   // the last launch re-armed the other half of the slot's counters
    HIPCHECK(hipEventRecord(sl.evDone, sl.stream));
    return PT_OK;
}

// iterations [b0, b1) of the slot's batch of `count` into the accumulator (or nowhere: `discard`), on the caller's stream
int commit_range(Slot &sl, int count, int b0, int b1, bool discard) {
    if (R().nLocal > 0) {
        float *snap = discard ? nullptr : R().snapTarget;
        if (snap && R().snapWait) {
            HIPCHECK(hipStreamWaitEvent(R().stream, R().snapWait, 0));
            R().snapWait = nullptr;
        }
        const int compact = (R().flags & PT_FLAG_ACCUM_SHARD_ROWS) ? 1 : 0;
        const dim3 grid((R().nLocal + kBlock - 1) / kBlock);
        float *const mom = R().moments.p;      // PT_FLAG_MOMENTS: the <true> instantiations, which also square what they add
        if (b1 == b0 + 1)      // one iteration of the batch (the reference's protocol over a batch traced ahead): the light kernel
            hipLaunchKernelGGL(mom ? k_commit_one<true> : k_commit_one<false>, grid, dim3(kBlock), 0, R().stream, R().prm, R().image, sl.contrib.p,
                               sl.hitMask.p, compact, b0, discard ? 1 : 0, snap, mom);
        else
            hipLaunchKernelGGL(mom ? k_commit<true> : k_commit<false>, grid, dim3(kBlock), 0, R().stream, R().prm, R().image, sl.contrib.p, sl.hitMask.p,
                               count, compact, b0, b1, discard ? 1 : 0, snap, mom);
        HIPCHECK(hipGetLastError());
    }
    return PT_OK;
}

// PT_FLAG_TRACE_AHEAD: trace the batch that starts at iteration `first` into the next slot of the rotation and park it
int trace_ahead(int first) {
    int count = std::min(R().maxBatch, kIterEnd - first);
    if (!R().poses.empty()) {        // PT_FLAG_MOTION: a batch sees one pose, so it ends with its run
        count = std::min(count, motion_run_end(first) - first);
        activate_step(R(), motion_step(first));
    }
    const int slot = (int)(R().seq % R().nslots);
    int rc = trace_batch(R().slot[slot], first, count);
    if (rc) return rc;
    R().ahead.push_back({slot, first, count, 0, false});
    R().seq += 1;
    return PT_OK;
}

// ... and drop what is parked: the caller asked for something else.  The iterations not yet committed are consumed without
// being added, which leaves the slots' buffers zeroed as every batch expects to find them.
int discard_ahead() {
    for (const State::Parked &p : R().ahead) {
        Slot &sl = R().slot[p.slot];
        HIPCHECK(hipStreamWaitEvent(R().stream, sl.evDone, 0));
        int rc = commit_range(sl, p.count, p.next, p.count, true);
        if (rc) return rc;
        HIPCHECK(hipEventRecord(sl.evCommitted, R().stream));
    }
    R().ahead.clear();
    return PT_OK;
}

// Process exit with work in flight (an exception in the host between pt_iterate and pt_free, an interpreter that is torn down
// with a live renderer): the streams are drained and everything is released BEFORE the HIP runtime's own exit handlers run --
// this handler is registered after the library's first HIP call, and exit handlers run in reverse order of registration --
// so that no launch of this process is still executing when its queues, its code object and its memory go away.
extern "C" void pt_free(void);
extern "C" void pt_group_destroy(PtGroup *g);
void free_renderer(bool keepHistory = false);
void exit_handler() {
    for (;;) {                                    // groups the host forgot: their members' renderers, threads, RCCL communicators, buffers
        PtGroup *g = nullptr;
        {
            std::lock_guard<std::mutex> lock(g_groupMutex);
            if (!g_groups.empty()) g = g_groups.back();
        }
        if (!g) break;
        pt_group_destroy(g);
    }
    pt_free();                                    // the calling thread's current context (normally the default one) + the scan library
    std::vector<State *> all;
    {
        std::lock_guard<std::mutex> lock(g_ctxMutex);
        all = g_contexts;
    }
    all.push_back(&g_default);
    for (State *st : all) {                       // ... and every other renderer the process still holds
        t_ctx = st;
        free_renderer();
    }
    t_ctx = &g_default;
}
void register_exit_handler() {
    static std::once_flag once;                   // (several host threads may drive contexts of their own)
    std::call_once(once, [] { atexit(exit_handler); });
}

// ---- the denoiser (pt_denoise.h) ---------------------------------------------------------------------------------------------------
// which form of k_atrous a level takes: the plain gather, or the LDS-tiled one with one or two rows per wave
enum { kAtrousAuto = 0, kAtrousGather = 1, kAtrousTiled4 = 2, kAtrousTiled8 = 3 };

// the kernel of a level by (first, last, bytes, form): 12 per filter, and the guided one's three <false, true, ., BYTES>
template <class Filter, bool F, bool L, bool BYTES = false>
const void *atrous_forms(int form) {
    if (form == kAtrousGather) return reinterpret_cast<const void *>(k_atrous_gather<Filter, F, L, BYTES>);
    if (form == kAtrousTiled4) return reinterpret_cast<const void *>(k_atrous_tiled<Filter, F, L, 1, BYTES>);
    return reinterpret_cast<const void *>(k_atrous_tiled<Filter, F, L, 2, BYTES>);
}
template <class Filter>
const void *atrous_kernel(bool first, bool last, bool bytes, int form) {
    if constexpr (Filter::kVariance)
        if (bytes) return atrous_forms<Filter, false, true, true>(form);
    return first ? (last ? atrous_forms<Filter, true, true>(form) : atrous_forms<Filter, true, false>(form))
                 : (last ? atrous_forms<Filter, false, true>(form) : atrous_forms<Filter, false, false>(form));
}

// ... and of a description that differs from its filter in the last level's store alone (AtrousDemod): <false, true, ., BYTES> and no other
template <class Last>
const void *atrous_last_kernel(bool bytes, int form) {
    return bytes ? atrous_forms<Last, false, true, true>(form) : atrous_forms<Last, false, true>(form);
}

int denoise_refusals(const char *who) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "%s before pt_init", who);
    if (R().prm.shardCount > 1 || (R().flags & PT_FLAG_ACCUM_SHARD_ROWS))
        return fail(PT_ERR_INVALID, "%s: the renderer holds a row shard, its accumulator is not a frame", who);
    if (R().flags & PT_FLAG_MOTION)
        return fail(PT_ERR_INVALID, "%s: the renderer was initialised with PT_FLAG_MOTION (a first-hit guide has no single pose)", who);
    return PT_OK;
}

// dynamic LDS k_gbuffer needs for the renderer's scene: the lanes' mesh traversal stacks (a launch holds at most 64 KB)
size_t guide_stack_bytes() { return guideStackBytes(R().mesh, R().meshStackNeed); }

// the guide buffers of iteration `guideIter`, on the caller's stream (cached until pt_init / pt_free); ms: the kernel's time, 0 when cached
int ensure_guides(int guideIter, float *ms) {
    if (ms) *ms = 0.0f;
    if (guideIter < 1 || guideIter >= kIterEnd) return fail(PT_ERR_INVALID, "guide_iter must be 1..4194303");
    const size_t P = (size_t)R().P;
    if (!R().dnPosT.p) PTCHECK(R().dnPosT.alloc(P));
    if (!R().dnNrmId.p) PTCHECK(R().dnNrmId.alloc(P));
    if (R().dnGuideIter == guideIter) return PT_OK;
    const size_t stackBytes = guide_stack_bytes();
    if (stackBytes > 64 * 1024) return fail(PT_ERR_INVALID, "guide buffers: a mesh hierarchy needs %d stack levels", R().meshStackNeed);
    Event ev[2];
    if (ms) {
        for (Event &e : ev) PTCHECK(e.create(hipEventDefault));
        HIPCHECK(hipEventRecord(ev[0], R().stream));
    }
    R().dnGuideIter = 0;
    hipLaunchKernelGGL(k_gbuffer, dim3((unsigned)((P + kBlock - 1) / kBlock)), dim3(kBlock), stackBytes, R().stream, R().prm, R().tab.dgeoms.p,
                       reinterpret_cast<const float4 *>(R().tab.dMeshRecs.p), guideIter, R().dnPosT.p, R().dnNrmId.p);
    HIPCHECK(hipGetLastError());
    if (ms) {
        HIPCHECK(hipEventRecord(ev[1], R().stream));
        HIPCHECK(hipEventSynchronize(ev[1]));
        HIPCHECK(hipEventElapsedTime(ms, ev[0], ev[1]));
    }
    R().dnGuideIter = guideIter;
    return PT_OK;
}

// The levels of either filter (pt_denoise.h: a filter description) on the caller's stream, behind every committed iteration; the result is
// left in R().dnOut (packed RGB).  p: the caller's PtDenoiseParams or PtDenoiseVarParams, sigmaColour its first sigma; A: the filter's own
// members set, the rest is filled here.  form: kAtrousAuto is the product's choice per level; ms (or NULL): 1 + levels kernel times, k_gbuffer first.
// front(): what the filter puts between the guides and level 0; `blended`: it leaves level 0's input in R().dnPing[1], the half the level
// before level 0 would have written, so level 0 runs as a later level at step 1.
// bytesOut (the display path; a filter with a BYTES form): sendImageToPBO's bytes of the filtered mean go there instead -- device memory of
// P uchar4 -- written by the last level itself (`fused`, the product's way: k_atrous_*<AtrousGuided, false, true, ., true>, measured faster
// than the pair in profiles/display_cost.txt; R().dnOut is not touched then), or by k_to_rgba8 of R().dnOut behind it -- the test build's
// reference -- which belongs to the last level's time in `ms`.  A last level that reads the accumulators (levels 1, not blended) has no fused
// form and takes the two launches.
// Last: the description of the last level where it is not the filter's own (AtrousDemod: its Args extend the filter's, and the levels below
// the last are the filter's kernels over the part they share); such a run is always `blended`.
template <class Filter, class Last = Filter, class Params, class Front>
int atrous_run(typename Last::Args &A, int samples, const Params *p, float sigmaColour, int form, float *ms, const char *who, bool blended, Front front,
               uchar4 *bytesOut = nullptr, bool fused = true) {
    if (p->levels < 1 || p->levels > 8) return fail(PT_ERR_INVALID, "%s: levels must be 1..8", who);
    for (float sg : {sigmaColour, p->sigma_normal, p->sigma_position})
        if (!(sg > 0.0f)) return fail(PT_ERR_INVALID, "%s: a sigma must be > 0 (+inf switches its term off)", who);
    if (form < kAtrousAuto || form > kAtrousTiled8) return fail(PT_ERR_INVALID, "%s: unknown kernel form %d", who, form);
    constexpr bool ownLast = std::is_same<Filter, Last>::value;
    if (!ownLast && !blended) return fail(PT_ERR_INVALID, "%s: internal error: a last level of its own needs a blended level 0", who);
    PTCHECK(ensure_guides(p->guide_iter, ms));
    const size_t P = (size_t)R().P;
    const bool bytesFused = Filter::kVariance && bytesOut && fused && (p->levels > 1 || blended);
    if (!bytesFused && !R().dnOut.p) PTCHECK(R().dnOut.alloc(P * 3));
    for (int k = 0; k < 2 && k < p->levels - 1; ++k)
        if (!R().dnPing[k].p) PTCHECK(R().dnPing[k].alloc(P));
    PTCHECK(front());
    A.accum = R().image;
    A.posT = R().dnPosT.p; A.nrmId = R().dnNrmId.p;
    A.W = R().prm.W; A.H = R().prm.H;
    A.samples = (float)samples;
    A.invN = 1.0f / (p->sigma_normal * p->sigma_normal);
    A.invP = 1.0f / (p->sigma_position * p->sigma_position);
    Event ev[9];                    // (levels <= 8)
    if (ms)
        for (int i = 0; i <= p->levels; ++i) PTCHECK(ev[i].create(hipEventDefault));
    for (int i = 0; i < p->levels; ++i) {
        const bool first = i == 0 && !blended, last = i == p->levels - 1;
        A.step = 1 << i;
        Filter::hostColourScale(A, sigmaColour, i);
        A.cin = first ? nullptr : R().dnPing[(i + 1) & 1].p;
        A.cout = last ? nullptr : R().dnPing[i & 1].p;
        A.out3 = last ? R().dnOut.p : nullptr;
        if constexpr (Filter::kVariance)
            if (last && bytesFused) A.out8 = bytesOut;
        int f = form != kAtrousAuto ? form : (A.step <= Filter::kTiledMaxStep ? kAtrousTiled8 : kAtrousGather);
        unsigned long long grid = f == kAtrousGather ? atrousGridGather(A.W, A.H) : atrousGridTiled(A.W, A.H, A.step, f == kAtrousTiled4 ? 1 : 2);
        if (grid > 0x7fffffffull) {       // (a frame of few, very long rows at a large step: more tiles than a launch holds)
            f = kAtrousGather;
            grid = atrousGridGather(A.W, A.H);
        }
        void *kargs[] = {&A};       // (Last::Args begins with Filter::Args: a level below the last reads the part it knows)
        const void *kernel;
        if constexpr (ownLast) kernel = atrous_kernel<Filter>(first, last, last && bytesFused, f);
        else kernel = last ? atrous_last_kernel<Last>(bytesFused, f) : atrous_kernel<Filter>(false, false, false, f);
        if (ms) HIPCHECK(hipEventRecord(ev[i], R().stream));
        HIPCHECK(hipLaunchKernel(kernel, dim3((unsigned)grid), dim3(kBlock), kargs, 0, R().stream));
    }
    if (bytesOut && !bytesFused) {
        // sendImageToPBO's conversion of the filtered MEAN: k_to_rgba8 with one sample (x / 1 is exact)
        hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().dnOut.p, R().P, 1, bytesOut);
    }
    if (ms) {
        HIPCHECK(hipEventRecord(ev[p->levels], R().stream));
        HIPCHECK(hipEventSynchronize(ev[p->levels]));
        for (int i = 0; i < p->levels; ++i) HIPCHECK(hipEventElapsedTime(&ms[1 + i], ev[i], ev[i + 1]));
    }
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

// pt_denoise's levels (AtrousPlain).  kAtrousAuto: NOT measured yet for this filter -- profiles/denoise_cost.py is the measurement to run: the
// expectation is that the tiled form wins while a class's rows still share cache lines, and the gather, whose taps stay coalesced at every
// step, beyond.
int denoise_run(int samples, const PtDenoiseParams *p, size_t bytes, int form, float *ms, const char *who) {
    PTCHECK(denoise_refusals(who));
    if (!p || bytes != sizeof(PtDenoiseParams))
        return fail(PT_ERR_INVALID, "%s: the caller's PtDenoiseParams is %zu bytes, this library's %zu", who, p ? bytes : (size_t)0, sizeof(PtDenoiseParams));
    if (samples < 1) return fail(PT_ERR_INVALID, "%s: samples must be >= 1", who);
    AtrousArgs A;
    return atrous_run<AtrousPlain>(A, samples, p, p->sigma_color, form, ms, who, false, [] { return PT_OK; });
}

// a finished run's packed RGB and, asked for, its variance image to the host
int denoise_result_to_host(float *rgb_mean_host, float *var_host) {
    HIPCHECK(hipMemcpyAsync(rgb_mean_host, R().dnOut.p, (size_t)R().P * 3 * sizeof(float), hipMemcpyDeviceToHost, R().stream));
    if (var_host) HIPCHECK(hipMemcpyAsync(var_host, R().dnVar.p, (size_t)R().P * sizeof(float), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

int denoise_to_host(int samples, const PtDenoiseParams *p, size_t bytes, int form, float *ms, float *rgb_mean_host, const char *who) {
    if (!rgb_mean_host) return fail(PT_ERR_INVALID, "%s: null", who);
    PTCHECK(denoise_run(samples, p, bytes, form, ms, who));
    return denoise_result_to_host(rgb_mean_host, nullptr);
}

// ---- temporal reprojection (pt_temporal.h) -----------------------------------------------------------------------------------------------
// The old view's camera as k_temporal projects into it: camera_params takes `view` and `up` as given -- not unit, not orthogonal -- so the
// rows are the inverse of the 3 x 3 matrix [view | -right | -up], in double, rounded once: the exact inverse of cameraRayAt's pinhole map.
// (A singular basis -- view parallel to up -- gives rows that are not finite: every pixel then fails step 2 or 3 and has no history.)
TemporalCam temporal_camera(const KParams &k) {
    const double m[3][3] = {{k.view[0], -(double)k.right[0], -(double)k.up[0]},
                            {k.view[1], -(double)k.right[1], -(double)k.up[1]},
                            {k.view[2], -(double)k.right[2], -(double)k.up[2]}};
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    const double inv[3][3] = {{c00 / det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det},
                              {c01 / det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det},
                              {c02 / det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det}};
    TemporalCam c;
    for (int a = 0; a < 3; ++a) {
        c.e[a] = k.pos[a];
        c.r0[a] = (float)inv[0][a];
        c.r1[a] = (float)inv[1][a];
        c.r2[a] = (float)inv[2][a];
    }
    c.pixLenX = k.pixLenX; c.pixLenY = k.pixLenY; c.halfW = k.halfW; c.halfH = k.halfH;
    return c;
}

// PT_FLAG_OBJECT_HISTORY: the motion table between the geoms the history's view was rendered with and the coming view's (include/pt_amd.h,
// "object history"; tests/temporal_motion_ref.py restates it in float64).  Matrices are column-major, m[col * 4 + row]; every double
// operation is one IEEE operation in the order written (-ffp-contract=off holds for the host too).  An unmoved primitive's row holds the
// identity, which no kernel reads.  Answers whether a row has another state than 0.
bool motion_table(const PtGeom *then, const PtGeom *now, int n, std::vector<MotionRow> &rows) {
    rows.assign((size_t)(n > 0 ? n : 0), MotionRow{});
    bool any = false;
    for (int g = 0; g < n; ++g) {
        MotionRow &r = rows[(size_t)g];
        float *const G[3] = {r.g0, r.g1, r.g2};
        if (!memcmp(then[g].transform, now[g].transform, sizeof now[g].transform) &&
            !memcmp(then[g].inverseTransform, now[g].inverseTransform, sizeof now[g].inverseTransform)) {
            for (int k = 0; k < 3; ++k) { r.m[k][k] = 1.0f; G[k][k] = 1.0f; }
            r.state = 0;
            continue;
        }
        any = true;
        const float *T = then[g].transform, *Ti = now[g].inverseTransform;
        double A[3][4];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j)
                A[i][j] = (((double)T[0 + i] * (double)Ti[j * 4 + 0] + (double)T[4 + i] * (double)Ti[j * 4 + 1]) + (double)T[8 + i] * (double)Ti[j * 4 + 2]) +
                          (double)T[12 + i] * (double)Ti[j * 4 + 3];
        const double c[3][3] = {{A[1][1] * A[2][2] - A[1][2] * A[2][1], A[1][2] * A[2][0] - A[1][0] * A[2][2], A[1][0] * A[2][1] - A[1][1] * A[2][0]},
                                {A[0][2] * A[2][1] - A[0][1] * A[2][2], A[0][0] * A[2][2] - A[0][2] * A[2][0], A[0][1] * A[2][0] - A[0][0] * A[2][1]},
                                {A[0][1] * A[1][2] - A[0][2] * A[1][1], A[0][2] * A[1][0] - A[0][0] * A[1][2], A[0][0] * A[1][1] - A[0][1] * A[1][0]}};
        const double det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2];
        bool finite = true;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 4; ++j) { r.m[i][j] = (float)A[i][j]; finite = finite && std::isfinite(r.m[i][j]); }
            for (int j = 0; j < 3; ++j) { G[i][j] = (float)(c[i][j] / det); finite = finite && std::isfinite(G[i][j]); }
        }
        r.state = finite ? 1 : 2;
    }
    return any;
}

// k_temporal over the renderer and its context's history, on its stream: the blend of `samples` committed iterations with the history -- the
// halves a live history holds; none, or useHistory false: every pixel goes without -- into out (and outN: the capture and the moments form);
// needs the guides (ensure_guides).  ALBEDO (PT_FLAG_DEMOD_HISTORY): the blend of the albedo too, into outA.  A live history that holds a
// motion table (PT_FLAG_OBJECT_HISTORY with a primitive in another pose) takes the MOTION form; every other launch is what it was.
template <int FORM, bool ALBEDO = false>
int temporal_blend(float samples, float4 *out, float *outN, bool useHistory = true, float4 *outA = nullptr) {
    const State &S = R();
    const History &hs = S.hist;
    const bool live = useHistory && hs.live;
    TemporalArgs T;
    T.accum = S.image; T.moments = S.moments.p;
    T.posT = S.dnPosT.p; T.nrmId = S.dnNrmId.p;
    T.hc = live ? hs.hc[hs.cur].p : nullptr; T.hn = live ? hs.hn[hs.cur].p : nullptr;
    T.hpos = hs.hpos.p; T.hnrm = hs.hnrm.p;
    T.cam = hs.cam;
    T.W = S.prm.W; T.H = S.prm.H;
    T.samples = samples;
    T.out = out; T.outN = outN;
    T.ha = live && ALBEDO ? hs.ha[hs.cur].p : nullptr;
    T.asum = S.albedo.p; T.outA = outA; T.eps = PT_DEMOD_MIN_ALBEDO;
    if (ALBEDO && (!outA || !T.asum || (live && !hs.albedo))) return fail(PT_ERR_INVALID, "internal error: an albedo blend without its images");
    const bool motion = live && hs.motion.p != nullptr;
    T.motion = motion ? hs.motion.p : nullptr;
    T.motionN = motion ? (int)hs.motionHost.size() : 0;
    T.histCap = motion ? hs.cap : PT_TEMPORAL_MAX_HISTORY;
    const dim3 grid((unsigned)(((size_t)S.P + kBlock - 1) / kBlock));
    if (motion) hipLaunchKernelGGL((k_temporal<FORM, ALBEDO, true>), grid, dim3(kBlock), 0, S.stream, T);
    else hipLaunchKernelGGL((k_temporal<FORM, ALBEDO>), grid, dim3(kBlock), 0, S.stream, T);
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

// one form of k_temporal over arguments of the caller's, on the null stream (the test library's pt_test_temporal_motion)
template <int FORM, bool ALBEDO>
void temporal_motion_launch(bool motion, dim3 grid, const TemporalArgs &T) {
    if (motion) hipLaunchKernelGGL((k_temporal<FORM, ALBEDO, true>), grid, dim3(kBlock), 0, nullptr, T);
    else hipLaunchKernelGGL((k_temporal<FORM, ALBEDO, false>), grid, dim3(kBlock), 0, nullptr, T);
}

// PT_FLAG_OBJECT_HISTORY, behind the capture (or where none was due): the table between the poses the history is in and the coming view's
// geoms -- none where the context holds no history, where it was not captured under the flag, or where no primitive moved.
int refresh_motion(History &hs, bool flagged, const PtGeom *geoms, int ngeoms) {
    hs.motion.release();
    hs.motionHost.clear();
    hs.cap = PT_TEMPORAL_MAX_HISTORY;
    if (!flagged || !hs.live || hs.pose.empty() || (int)hs.pose.size() != ngeoms) return PT_OK;
    std::vector<MotionRow> rows;
    if (!motion_table(hs.pose.data(), geoms, ngeoms, rows)) return PT_OK;
    PTCHECK(hs.motion.upload(reinterpret_cast<const float4 *>(rows.data()), rows.size() * kMotionRowVec));
    hs.motionHost = std::move(rows);
    hs.cap = PT_OBJECT_HISTORY_MAX;
    return PT_OK;
}

// pt_init over a live PT_FLAG_TEMPORAL renderer that has committed R().committed >= 1 iterations: the old view's blend of ITS history with
// ITS samples becomes the context's history (k_temporal<true> into the other half of the ping-pong pair), its guide buffers of iteration 1
// -- the cached ones, or one k_gbuffer launch -- are handed over, and its camera is kept.  On the old renderer's stream, behind its commits.
int capture_history() {
    State &S = R();
    History &hs = S.hist;
    if (S.device >= 0) HIPCHECK(hipSetDevice(S.device));
    PTCHECK(ensure_guides(1, nullptr));
    const size_t P = (size_t)S.P;
    const int nxt = hs.live ? hs.cur ^ 1 : 0;
    if (!hs.hc[nxt].p) PTCHECK(hs.hc[nxt].alloc(P));
    if (!hs.hn[nxt].p) PTCHECK(hs.hn[nxt].alloc(P));
    // PT_FLAG_DEMOD_HISTORY: Ha' = (Ab, tot) beside them (pt_init keeps history only between renderers that agree on the flag)
    const bool withAlbedo = (S.flags & PT_FLAG_DEMOD_HISTORY) != 0;
    if (withAlbedo && !hs.ha[nxt].p) PTCHECK(hs.ha[nxt].alloc(P));
    // (S.committed, not `iterations`: pt_counters_reset zeroes that one and leaves the accumulators)
    if (withAlbedo) PTCHECK((temporal_blend<kTemporalCapture, true>((float)S.committed, hs.hc[nxt].p, hs.hn[nxt].p, true, hs.ha[nxt].p)));
    else PTCHECK(temporal_blend<kTemporalCapture>((float)S.committed, hs.hc[nxt].p, hs.hn[nxt].p));
    HIPCHECK(hipStreamSynchronize(S.stream));      // (the guides it read are released next)
    // (an exchange: the guides the history held until now -- the blend above has just read them -- are left to the renderer as buffers without
    // a content; pt_init frees them with it, the camera move renders the next view's guides into them)
    std::swap(hs.hpos, S.dnPosT);
    std::swap(hs.hnrm, S.dnNrmId);
    S.dnGuideIter = 0;
    hs.cam = temporal_camera(S.prm);
    hs.cur = nxt; hs.W = S.prm.W; hs.H = S.prm.H;
    hs.live = true;
    hs.albedo = withAlbedo;
    // PT_FLAG_OBJECT_HISTORY: the history is in this view's poses now (the table it was read through is replaced by the coming view's)
    if (S.flags & PT_FLAG_OBJECT_HISTORY) hs.pose = S.inGeoms;
    else hs.pose.clear();
    return PT_OK;
}

// PT_FLAG_DEMOD_HISTORY at two samples and more: the front as ONE launch, k_temporal<kTemporalFilterDemod, true>, or as the two it fuses,
// k_temporal<kTemporalFilter, true> and k_demodulate<true> -- the same bits.  Measured (profiles/demod_history_cost.txt): at 1280 x 720 the
// fused front takes 0.044 ms against the two launches' 0.051, at 1920 x 1080 0.074 against 0.089 -- ahead by 0.007 and 0.015 ms, several
// times the two-launch form's best-to-median spread of 0.001 and 0.002 ms.  The two launches stay in the test build alone
// (pt_test_temporal_albedo).
constexpr bool kDemodHistoryFused = true;

// ---- the spatial variance estimate (pt_spatial_var.h) -------------------------------------------------------------------------------------
enum { kSpatialGather = 0, kSpatialTiled = 1 };
// The form the product launches: measured (profiles/spatial_var_cost.txt) -- at 1280 x 720 the LDS tiles take 0.023 ms against the gather's 0.032
// where every pixel estimates (a renderer's first frame), 0.019 against 0.021 where one pixel in sixteen does (a view with history), both
// many times the gather's best-to-median spread of 0.0004 ms; at 1920 x 1080 0.043 against 0.064.  The gather stays in the test build alone.
constexpr int kSpatialForm = kSpatialTiled;

template <int RADIUS>
const void *spatial_kernel_of(int form) {
    return form == kSpatialTiled ? reinterpret_cast<const void *>(k_spatial_variance_tiled<RADIUS>)
                                 : reinterpret_cast<const void *>(k_spatial_variance_gather<RADIUS>);
}

// (a template, so that the form not taken is not instantiated)
template <int FORM>
const void *spatial_product_kernel() {
    if constexpr (FORM == kSpatialTiled) return reinterpret_cast<const void *>(k_spatial_variance_tiled<PT_SPATIAL_RADIUS>);
    else return reinterpret_cast<const void *>(k_spatial_variance_gather<PT_SPATIAL_RADIUS>);
}

// the product instantiates the shipped radius in the shipped form only; the test build every radius in both
const void *spatial_kernel(int radius, int form) {
#ifdef PT_TEST_API
    if (radius == 1) return spatial_kernel_of<1>(form);
    if (radius == 2) return spatial_kernel_of<2>(form);
    if (radius == 3) return spatial_kernel_of<3>(form);
    return nullptr;
#else
    if (radius != PT_SPATIAL_RADIUS || form != kSpatialForm) return nullptr;
    return spatial_product_kernel<kSpatialForm>();
#endif
}

int spatial_launch(SpatialArgs &A, int radius, int form, hipStream_t st) {
    const void *k = spatial_kernel(radius, form);
    if (!k) return fail(PT_ERR_INVALID, "spatial variance: radius %d in form %d is not in this build", radius, form);
    void *kargs[] = {&A};
    HIPCHECK(hipLaunchKernel(k, dim3(atrousGridGather(A.W, A.H)), dim3(kBlock), kargs, 0, st));
    return PT_OK;
}

// ---- albedo demodulation (pt_albedo.h) ------------------------------------------------------------------------------------------------------
// k_albedo for iterations first .. first + count - 1 of the renderer's scene, on its stream: no host synchronisation
int albedo_launch(int first, int count) {
    const State &S = R();
    AlbedoArgs A;
    A.prm = S.prm;
    A.ggeoms = S.tab.dgeoms.p; A.gmats = S.tab.dmats.p;
    A.meshRecs = reinterpret_cast<const float4 *>(S.tab.dMeshRecs.p);
    A.texGeom = S.tex ? S.tab.dTexGeom.p : nullptr;       // (a scene without a bound texture has no table)
    A.texDesc = S.tab.dTexDesc.p; A.texels = S.tab.dTexels.p; A.texUV = S.tab.dTexUV.p;
    A.firstIter = first; A.count = count;
    A.asum = S.albedo.p;
    hipLaunchKernelGGL(k_albedo, dim3((unsigned)(((size_t)S.P + kBlock - 1) / kBlock)), dim3(kBlock), guide_stack_bytes(), S.stream, A);
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

int demod_launch(DemodArgs &D, bool inplace, hipStream_t st) {
    const dim3 grid((unsigned)(((size_t)D.npix + kBlock - 1) / kBlock));
    if (inplace) hipLaunchKernelGGL(k_demodulate<true>, grid, dim3(kBlock), 0, st, D);
    else hipLaunchKernelGGL(k_demodulate<false>, grid, dim3(kBlock), 0, st, D);
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

// ---- the second moments and the variance-guided filter (pt_denoise.h, AtrousGuided) -----------------------------------------------------
int moments_refusals(const char *who) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "%s before pt_init", who);
    if (!R().moments.p) return fail(PT_ERR_INVALID, "%s: the renderer was initialised without PT_FLAG_MOMENTS", who);
    return PT_OK;
}

// PT_FLAG_DISPLAY_FILTER: the one setting of the display path (include/pt_amd.h)
const PtDenoiseVarParams kDisplayParams = {PT_DISPLAY_LEVELS, PT_DISPLAY_GUIDE_ITER, PT_DISPLAY_SIGMA_LUM, PT_DISPLAY_SIGMA_NORMAL, PT_DISPLAY_SIGMA_POSITION};

// pt_denoise_var's levels (AtrousGuided; atrous_run): packed RGB in R().dnOut, the filtered variance in R().dnVar when `wantVar`; bytesOut,
// fused (the display path; not with wantVar): atrous_run's.
int denoise_var_run(int samples, const PtDenoiseVarParams *p, size_t bytes, int form, bool wantVar, float *ms, const char *who,
                    uchar4 *bytesOut = nullptr, bool fused = true) {
    PTCHECK(moments_refusals(who));
    PTCHECK(denoise_refusals(who));      // (the moments need the whole frame, so this adds PT_FLAG_MOTION's refusal alone)
    if (!p || bytes != sizeof(PtDenoiseVarParams))
        return fail(PT_ERR_INVALID, "%s: the caller's PtDenoiseVarParams is %zu bytes, this library's %zu", who, p ? bytes : (size_t)0, sizeof(PtDenoiseVarParams));
    if (R().flags & PT_FLAG_SPATIAL_VARIANCE) {
        if (samples < 1) return fail(PT_ERR_INVALID, "%s: samples must be >= 1", who);
    } else if (samples < 2) {
        return fail(PT_ERR_INVALID, "%s: samples must be >= 2 (a variance needs two)", who);
    }
    // PT_FLAG_TEMPORAL with history: level 0 reads the blend of the reprojected history with the accumulators (k_temporal<kTemporalFilter>)
    const History &hist = R().hist;
    const bool temporal = (R().flags & PT_FLAG_TEMPORAL) && hist.live && hist.W == R().prm.W && hist.H == R().prm.H;
    // PT_FLAG_SPATIAL_VARIANCE: the counts are Nh + samples, so only a one-sample frame holds a pixel below PT_SPATIAL_MIN_COUNT; level 0 then reads
    // the blend's colour with the variance k_spatial_variance_* gives it (pt_spatial_var.h).  From two samples on: today's launches.
    const bool spatial = samples < 2;
    // PT_FLAG_DEMODULATE (pt_albedo.h): k_demodulate between the front and level 0, which then always runs as a later level at step 1, and
    // AtrousDemod's last level, which multiplies the albedo back
    const bool demod = (R().flags & PT_FLAG_DEMODULATE) != 0;
    // PT_FLAG_DEMOD_HISTORY while the context holds history of the flagged kind (pt_temporal.h, ALBEDO): the blends also leave (Ab, tot) in
    // R().dnAlbedo, k_demodulate divides by it (samples 1: x / 1 is exact), and below PT_DEMOD_HISTORY_MIN_OWN samples the last level multiplies
    // it back -- from there on the renderer's own sums.  Without live history: PT_FLAG_DEMODULATE's launches.
    const bool demodHist = temporal && (R().flags & PT_FLAG_DEMOD_HISTORY) && hist.albedo;
    AtrousDemodArgs A;                 // (AtrousVarArgs and, behind them, what AtrousDemod's last level alone reads)
    A.moments = R().moments.p;
    A.samplesM1 = (float)(samples - 1);
    A.asum = R().albedo.p; A.demodN = (float)samples; A.demodEps = PT_DEMOD_MIN_ALBEDO;
    if (demodHist && samples < PT_DEMOD_HISTORY_MIN_OWN) { A.asum = R().dnAlbedo.p; A.demodN = 1.0f; }
    bool frontDemodulated = false;     // (the fused front has divided already)
    const auto prepare = [&]() -> int {
        if (wantVar && !R().dnVar.p) PTCHECK(R().dnVar.alloc((size_t)R().P));
        A.outVar = wantVar ? R().dnVar.p : nullptr;       // (read by a last level alone)
        if (!temporal && !spatial) return PT_OK;
        if (!R().dnPing[1].p) PTCHECK(R().dnPing[1].alloc((size_t)R().P));
        if (!spatial && demodHist) {
            frontDemodulated = kDemodHistoryFused;
            return temporal_blend<kDemodHistoryFused ? kTemporalFilterDemod : kTemporalFilter, true>((float)samples, R().dnPing[1].p, nullptr, true, R().dnAlbedo.p);
        }
        if (!spatial) return temporal_blend<kTemporalFilter>((float)samples, R().dnPing[1].p, nullptr);
        // the moments image goes into dnPing[0], which level 0 overwrites only afterwards
        if (!R().dnPing[0].p) PTCHECK(R().dnPing[0].alloc((size_t)R().P));
        if (demodHist) PTCHECK((temporal_blend<kTemporalMoments, true>((float)samples, R().dnPing[0].p, R().dnCount.p, true, R().dnAlbedo.p)));
        else PTCHECK(temporal_blend<kTemporalMoments>((float)samples, R().dnPing[0].p, R().dnCount.p, temporal));
        SpatialArgs B;
        B.m4 = R().dnPing[0].p; B.cnt = R().dnCount.p;
        B.posT = R().dnPosT.p; B.nrmId = R().dnNrmId.p;
        B.W = R().prm.W; B.H = R().prm.H;
        B.invN = 1.0f / (p->sigma_normal * p->sigma_normal);      // (atrous_run's, which has checked the sigmas)
        B.invP = 1.0f / (p->sigma_position * p->sigma_position);
        B.out = R().dnPing[1].p;
        return spatial_launch(B, PT_SPATIAL_RADIUS, kSpatialForm, R().stream);
    };
    if (!demod) return atrous_run<AtrousGuided>(A, samples, p, p->sigma_lum, form, ms, who, temporal || spatial, prepare, bytesOut, fused);
    return atrous_run<AtrousGuided, AtrousDemod>(A, samples, p, p->sigma_lum, form, ms, who, true, [&]() -> int {
        PTCHECK(prepare());
        if (frontDemodulated) return PT_OK;
        if (!R().dnPing[1].p) PTCHECK(R().dnPing[1].alloc((size_t)R().P));
        DemodArgs D;
        D.accum = R().image; D.moments = R().moments.p;
        D.img = R().dnPing[1].p; D.asum = R().albedo.p;
        D.npix = R().P;
        D.samples = (float)samples; D.samplesM1 = (float)(samples - 1); D.eps = PT_DEMOD_MIN_ALBEDO;
        if (demodHist) {      // in place on the blend (or on the estimate made of it), by the blended albedo as a mean of one
            D.asum = R().dnAlbedo.p; D.samples = 1.0f; D.samplesM1 = 0.0f;
            return demod_launch(D, true, R().stream);
        }
        return demod_launch(D, spatial, R().stream);      // (in place on the image k_spatial_variance_* left, or from the accumulators)
    }, bytesOut, fused);
}

// PT_FLAG_DISPLAY_FILTER: the bytes of `samples` committed iterations as the display sees them, into device memory, on the renderer's stream
// behind everything enqueued: pt_denoise_var_rgba8's with the shipped setting, or -- one sample has no variance -- the plain conversion
// (not under PT_FLAG_SPATIAL_VARIANCE, which estimates one from the neighbours: the first frame is filtered too).
// pt_init allocated every buffer this touches; nothing here waits for the device.
int display_bytes(int samples, uchar4 *out, const char *who, int form = kAtrousAuto, bool fused = true, float *ms = nullptr) {
    if (samples < 2 && !(R().flags & PT_FLAG_SPATIAL_VARIANCE)) {
        hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().image, R().P, samples, out);
        HIPCHECK(hipGetLastError());
        return PT_OK;
    }
    return denoise_var_run(samples, &kDisplayParams, sizeof kDisplayParams, form, false, ms, who, out, fused);
}

int denoise_var_to_host(int samples, const PtDenoiseVarParams *p, size_t bytes, int form, float *ms, float *rgb_mean_host, float *var_host, const char *who) {
    if (!rgb_mean_host) return fail(PT_ERR_INVALID, "%s: null", who);
    PTCHECK(denoise_var_run(samples, p, bytes, form, var_host != nullptr, ms, who));
    return denoise_result_to_host(rgb_mean_host, var_host);
}


// ---- the noise statistics and the loop that renders until they pass (pt_noise.h) ------------------------------------------------------------
// a threshold or a luminance floor: finite and > 0
bool noise_positive(float v) { return v > 0.0f && v <= std::numeric_limits<float>::max(); }

// k_noise_stats over `accum` / `moments` on stream `st`: zero the two words, the kernel, and -- `host` given -- their copy to the host
int noise_launch(const float *accum, const float *moments, int W, int H, int samples, float lumFloor, float thr2, uint32_t *frame, float *tileMap,
                 uint32_t *host, hipStream_t st, int tilesPerWave = kNoiseTilesPerWave) {
    const long long tx = (W + kNoiseTile - 1) / kNoiseTile, ty = (H + kNoiseTile - 1) / kNoiseTile;
    if (tx * ty > 0x3fffffffll) return fail(PT_ERR_INVALID, "noise statistics: more than 2^30 tiles");
    const int tiles = (int)(tx * ty), perBlock = 4 * tilesPerWave;
    HIPCHECK(hipMemsetAsync(frame, 0, 2 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_noise_stats, dim3((tiles + perBlock - 1) / perBlock), dim3(kBlock), 0, st, accum, moments, W, H, (int)tx, tiles, tilesPerWave,
                       (float)samples, (float)(samples - 1), lumFloor, thr2, frame, tileMap);
    HIPCHECK(hipGetLastError());
    if (host) HIPCHECK(hipMemcpyAsync(host, frame, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return PT_OK;
}

// what the two words say, judged with the fraction `frac` of tiles that may stay unconverged
void noise_fill(PtNoiseStats *out, int W, int H, int samples, float thr2, const uint32_t *words, float frac) {
    out->samples = samples;
    out->tiles_x = (W + kNoiseTile - 1) / kNoiseTile;
    out->tiles_y = (H + kNoiseTile - 1) / kNoiseTile;
    out->tiles = (int64_t)out->tiles_x * out->tiles_y;
    out->unconverged = (int64_t)words[0];
    memcpy(&out->max_rel_var, &words[1], sizeof(float));
    out->thr2 = thr2;
    out->converged = out->unconverged <= (int64_t)std::floor((double)frac * (double)out->tiles) ? 1 : 0;
}

int noise_buffers() {
    if (!R().noiseFrame.p) PTCHECK(R().noiseFrame.alloc(2));
    if (!R().noiseHost) PTCHECK(R().noiseHost.alloc(4, hipHostMallocDefault));
    for (Event &e : R().noiseEv)
        if (!e) PTCHECK(e.create(hipEventDisableTiming));
    return PT_OK;
}

// one check of the accumulator as the caller's stream will have it behind everything enqueued so far: the kernel, the copy of its words into
// page-locked copy `k`, the event
int noise_enqueue_check(int k, int samples, float lumFloor, float thr2) {
    PTCHECK(noise_launch(R().image, R().moments.p, R().prm.W, R().prm.H, samples, lumFloor, thr2, R().noiseFrame.p, nullptr, R().noiseHost + 2 * k,
                         R().stream));
    HIPCHECK(hipEventRecord(R().noiseEv[k], R().stream));
    return PT_OK;
}

}  // namespace

// =====================================================================================================
// C ABI (the library is built with -fvisibility=hidden: these entry points are all it exports)
// =====================================================================================================
#pragma GCC visibility push(default)
extern "C" {

const char *pt_last_error(void) { return g_err.c_str(); }
int pt_device_count(void) { return count_devices(); }
int pt_abi_version(void) { return PT_AMD_ABI_VERSION; }

void pt_free(void) {
    // the scan library's per-stream workspaces (allocated on first use, with or without a renderer)
    scan_release();
    free_renderer();
}

}  // extern "C"
#pragma GCC visibility pop
namespace {
// everything pt_init allocated (pt_free, and pt_init's own restart)
void free_renderer(bool keepHistory) {
    if (!keepHistory) R().hist = History();        // (pt_init alone keeps it: a re-initialisation of a PT_FLAG_TEMPORAL renderer)
    // pathtraceFree before the first Init (src/main.cpp:91-94) must be a no-op
    if (R().holds_nothing()) return;
    if (R().device >= 0 && R().nslots > 0) (void)hipSetDevice(R().device);     // (a host that switched devices in between)
    // wait for everything, then let go: hipFree synchronises by itself, the destruction of a stream does not wait in the same way
    for (int i = 0; i < kMaxSlots; ++i)
        if (R().slot[i].stream) (void)hipStreamSynchronize(R().slot[i].stream);
    (void)hipStreamSynchronize(R().stream);
    if (R().pinnedHost) (void)hipHostUnregister(R().pinnedHost);
    // ... and everything else: the move-assignment below releases what the owners of State and its Slots hold (pt_owned.h)
    {   // (what is registered outlives the renderer: see State::reg)
        const Registered keep = R().reg;
        History keepHist = std::move(R().hist);
        R() = State();
        R().hist = std::move(keepHist);
        R().reg = keep;
    }
}

// The end of pt_init, and of the camera move: what depends on the plan's scalars and on which camera tables the device holds -- the kernels'
// LDS attributes, the persistent grids, and the camera-ray launch's column rotation (KParams::tilesPerRow).
int size_launches(State &S) {
    if (S.ldsBytes > 64 * 1024) {
        HIPCHECK(hipFuncSetAttribute(S.kernFirst, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.ldsBytes));
        HIPCHECK(hipFuncSetAttribute(S.kernNext, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.ldsBytes));
    }
    if (S.mesh)
        for (int first = 0; first < 2; ++first) {
            const void *kw = walk_kernel(first != 0, first && S.dof);
            if (S.ldsWalk > 64 * 1024) HIPCHECK(hipFuncSetAttribute(kw, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.ldsWalk));
            PTCHECK(persistent_grid(kw, S.ldsWalk, true, first ? &S.gridWalkFirst : &S.gridWalk));
        }
    for (int first = 0; first < 2; ++first) {
        int &grid = first ? S.gridFirst : S.grid;
        PTCHECK(persistent_grid(first ? S.kernFirst : S.kernNext, first ? S.ldsBytes : S.ldsBytesNext, false, &grid));
        if (grid > S.numTilesMax) grid = S.numTilesMax;
        grid = (grid / kSub) * kSub;      // T % kSub == blockIdx % kSub for every tile T of a workgroup (kSub: a multiple of the mesh scenes' 4 too)
        if (grid < kSub) grid = kSub;
    }
    // Camera-ray bounce: tile T covers pixels 256 T ... of the row-major frame and a workgroup owns the tiles b, b + grid,
    // ...  When the grid shares a factor with the tiles per row (1280 workgroups, 5 tiles per 1280-pixel row) a workgroup
    // stays in few column bands of the frame, and the bands outside the scene rectangle finish 15x earlier than the
    // others.  Either the grid can be made coprime to the tiles per row (both must stay multiples of kSub, so only for an
    // odd tile count per row), or the kernel rotates the k-th tile of a workgroup k bands to the right inside its row,
    // which needs a grid that is a multiple of the tiles per row (k_bounce<true, .>).
    // (the packed work list of camera rays has no column bands: nothing to rotate)
    const KParams &k = S.prm;
    S.prm.tilesPerRow = 0;
    if (k.Wp / kBlock > 1 && S.tab.dCamPix.p == nullptr) {
        const int perRow = k.Wp / kBlock;
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        if (gcd(perRow, kSub) == 1) {
            for (int tries = 0; tries < 64 && S.gridFirst > kSub && gcd(S.gridFirst, perRow) != 1; ++tries) S.gridFirst -= kSub;
        } else {
            const int unit = perRow / gcd(perRow, kSub) * kSub;        // lcm(perRow, kSub)
            if (S.gridFirst >= 4 * unit) {
                S.gridFirst = S.gridFirst / unit * unit;
                S.prm.tilesPerRow = perRow;
            }
        }
    }
    return PT_OK;
}

// The old view of a renderer that goes (pt_init) or moves on (the camera move), keepHistory: the history is to live on.  Is a capture due?
// Not without committed samples: the history lives on as it is.  And not for an old view whose scene k_gbuffer cannot trace -- a mesh
// hierarchy deeper than its 64 KB of stacks, the one thing pt_gbuffer answers PT_ERR_INVALID to: it has no guides to reproject through, the
// history ends there (keepHistory is cleared), and the call goes on.
bool capture_due(bool &keepHistory) {
    if (keepHistory && R().committed >= 1 && guide_stack_bytes() > 64 * 1024) keepHistory = false;
    return keepHistory && R().committed >= 1;
}

// ... and the capture where it is due: the old view becomes the context's history.  What is left to fail in it is a HIP call: PT_ERR_HIP,
// which leaves the context without a renderer like every other one of pt_init's.  who: the message's prefix.
int retire_view(bool &keepHistory, const char *who) {
    if (!capture_due(keepHistory)) return PT_OK;
    const int rc = capture_history();
    if (!rc) return PT_OK;
    free_renderer();
    return rc == PT_ERR_INVALID ? fail(PT_ERR_HIP, "%s: the capture of the old view failed: %s", who, std::string(g_err).c_str()) : rc;
}

// PT_FLAG_OBJECT_HISTORY: does a pt_init call describe the objects the live renderer was initialised with?  ngeoms, every geom's type and
// materialid, nmats and the materials' bytes, and what is registered now against the renderer's own copies (registered_mismatch: byte for
// byte, no hash).  translation, rotation, scale and the three matrices may differ.
bool same_objects(const State &S, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, const Registered &reg) {
    if (ngeoms != (int)S.inGeoms.size() || nmats != (int)S.inMats.size()) return false;
    for (int g = 0; g < ngeoms; ++g)
        if (geoms[g].type != S.inGeoms[(size_t)g].type || geoms[g].materialid != S.inGeoms[(size_t)g].materialid) return false;
    if (nmats > 0 && memcmp(mats, S.inMats.data(), (size_t)nmats * sizeof(PtMaterial))) return false;
    return registered_mismatch(reg, S.initReg) == nullptr;
}

// What the renderer's slots, accumulators and walks share whatever the plan's tables hold -- the allocations pt_init sized by a plan and the
// launches' common shape: do two plans agree on it?  NULL, or the name of the first member that differs.  The camera move asks it of the new
// camera's plan against the renderer (a difference: the full call); PT_FLAG_MOTION of every step against step 0 (a difference: refused).
const char *slots_mismatch(const PlanScalars &a, const PlanScalars &b) {
    if (a.mesh != b.mesh) return "mesh";
    if (a.dof != b.dof) return "dof";
    if (a.walkMeshLds != b.walkMeshLds) return "walkMeshLds";
    if (a.flags != b.flags) return "flags";
    if (a.nslots != b.nslots) return "nslots";
    if (a.maxBatch != b.maxBatch) return "maxBatch";
    if (a.poolCap != b.poolCap || a.poolChunks != b.poolChunks || a.prm.poolChunks != b.prm.poolChunks) return "the path pools' size";
    if (a.prm.chunkShift != b.prm.chunkShift) return "the path pools' chunk size";
    if (a.prm.histBits != b.prm.histBits) return "the path pools' layout (history bits)";
    if (a.meshHitWords != b.meshHitWords) return "meshHitWords";
    if (a.prm.contribLocal != b.prm.contribLocal) return "contribLocal";
    if (a.nLocal != b.nLocal || a.P != b.P) return "the frame";
    return nullptr;
}

// The dynamic-LDS attribute of every kernel the renderer's poses launch, set to the largest value any pose needs (size_launches sets each
// pose's own as it goes; poses that share a kernel would leave the last one's).  A renderer of one pose: what size_launches set.
int lds_attributes(State &S) {
    if (S.poses.empty()) return PT_OK;
    std::map<const void *, size_t> need;
    const int was = S.step;
    for (int s = 0; s < (int)S.poses.size(); ++s) {
        activate_step(S, s);
        for (const void *k : {S.kernFirst, S.kernNext}) need[k] = std::max(need[k], S.ldsBytes);
        if (S.mesh)
            for (int first = 0; first < 2; ++first) {
                const void *kw = walk_kernel(first != 0, first && S.dof);
                need[kw] = std::max(need[kw], S.ldsWalk);
            }
    }
    activate_step(S, was);
    for (const auto &kv : need)
        if (kv.second > 64 * 1024) HIPCHECK(hipFuncSetAttribute(kv.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kv.second));
    return PT_OK;
}

// a plan's tables in device bytes as pt_init allocates them; `invariant`: the camera-invariant ones (PT_FLAG_MOTION holds them once) or the rest
size_t table_bytes(ScenePlan &plan, bool invariant, long long *buffers = nullptr) {
    size_t bytes = 0;
    SceneTables none;
    (void)none.for_each(nullptr, plan, plan.mesh, plan.grouped, [&](const auto &, const auto *, const auto &table, TableRule rule) {
        if (rule.cameraInvariant != invariant || !rule.allocated(table.size())) return (int)PT_OK;
        bytes += rule.allocated(table.size()) * sizeof(table[0]);
        if (buffers) *buffers += 1;
        return (int)PT_OK;
    });
    return bytes;
}

// PT_FLAG_MOTION holds the camera-invariant tables once by leaving them in State::tab when poses are exchanged (exchange_pose names them):
// is that list the set SceneTables::for_each marks camera-invariant?  A table marked so and not named there would be null in every pose but
// the first.
bool invariant_tables_are_the_exchanged_ones(SceneTables &tab, ScenePlan &plan) {
    bool ok = true;
    int n = 0;
    (void)tab.for_each(nullptr, plan, true, true, [&](const auto &buf, const auto *, const auto &, TableRule rule) {
        if (!rule.cameraInvariant) return (int)PT_OK;
        n += 1;
        const void *at = &buf;
        if (at != (const void *)&tab.dTexels && at != (const void *)&tab.dMeshRecs) ok = false;
        return (int)PT_OK;
    });
    return ok && n == 2;
}

// the host's copies of the camera-invariant tables, once the device holds them
void drop_camera_invariant(SceneTables &tab, ScenePlan &plan) {
    (void)tab.for_each(nullptr, plan, plan.mesh, plan.grouped, [](const auto &, const auto *, auto &table, TableRule rule) {
        if (rule.cameraInvariant) std::decay_t<decltype(table)>().swap(table);
        return (int)PT_OK;
    });
}

int camera_faces_device(CameraGroups &G, const CameraResolve &cr, hipStream_t st, DevBuf<uint32_t> &pix, DevBuf<signed char> &face, float *ms);

// The device half of pt_init.  The scene is planned on the host first (pt_scene_plan.h: plan_scene), and a scene that is refused there --
// every PT_ERR_INVALID -- has touched nothing: no allocation made or released, the renderer that was there still initialised and usable.
// Only then the old renderer goes, and what can still fail (PT_ERR_NO_GPU, PT_ERR_HIP: the memory budget, which has to see the memory the
// old renderer gave back) leaves the context without a renderer.
// o: the options made effective; reg: what the scene's meshes, textures and height maps are -- what is registered now (pt_init), or what
// the live renderer was initialised with (the camera move's slow path); by value: the renderer that holds them goes.
int init_renderer(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions &o,
                  const Registered reg) {
    // PT_AMD_INIT_PHASES (measurements only: profiles/set_camera_cost.py): the host's clock around the call's phases, each ended by a
    // device synchronise of its own, printed to stderr
    const bool phases = env_flag("PT_AMD_INIT_PHASES");
    double phaseMs[5] = {0, 0, 0, 0, 0};
    auto phaseT0 = std::chrono::steady_clock::now();
    const auto phase_end = [&](int i) {
        if (!phases) return;
        if (i > 0) (void)hipDeviceSynchronize();
        const auto t = std::chrono::steady_clock::now();
        phaseMs[i] = std::chrono::duration<double, std::milli>(t - phaseT0).count();
        phaseT0 = t;
    };
    // PT_FLAG_MOTION: `geoms` holds PT_MOTION_STEPS scenes of ngeoms records; every step is planned like a call of its own before anything
    // is touched.  `plan` is step 0's -- the pose the renderer starts in, and without the flag the one there is --, `later` the others'.
    const int steps = (o.flags & PT_FLAG_MOTION) ? PT_MOTION_STEPS : 1;
    struct Planned { ScenePlan plan; const void *kernFirst = nullptr, *kernNext = nullptr; };
    // ... and the work list's face certificates, nearly all of a plan's host time, are evaluated on the device for every step, as the
    // camera move evaluates them (k_camera_faces through SceneIn::faces: the host's values, bit for bit), on a stream and in scratch
    // buffers of this call's own -- nothing of the live renderer is touched.  (PT_AMD_MOTION_HOST_FACES, measurements only: on the host;
    // without a device the host evaluates them too, and the call ends with PT_ERR_NO_GPU below as it always did.)
    const bool deviceFaces = steps > 1 && !env_flag("PT_AMD_MOTION_HOST_FACES") && count_devices() >= 1;
    Stream faceStream;
    DevBuf<uint32_t> facePix;
    DevBuf<signed char> faceBytes;
    struct DeviceGuard {      // the device current at the call, put back where planning ends in a refusal
        int prev = -1;
        bool armed = false;
        ~DeviceGuard() { if (armed && prev >= 0) (void)hipSetDevice(prev); }
    } deviceGuard;
    if (deviceFaces) {
        register_exit_handler();
        HIPCHECK(hipGetDevice(&deviceGuard.prev));
        deviceGuard.armed = true;
        if (o.device >= 0) HIPCHECK(hipSetDevice(o.device));
        PTCHECK(faceStream.create(hipStreamNonBlocking));
    }
    const auto plan_step = [&](const PtGeom *g, Planned &out) -> int {
        ScenePlan &plan = out.plan;
        SceneIn in(cam, g, ngeoms, mats, nmats, traceDepth, o, reg);
        if (deviceFaces)
            in.faces = [&](CameraGroups &G, const CameraResolve &cr) { return camera_faces_device(G, cr, faceStream, facePix, faceBytes, nullptr); };
        PTCHECK(plan_scene(in, plan));
        PTCHECK(resolve_bounce_kernel(plan, true, &out.kernFirst));
        PTCHECK(resolve_bounce_kernel(plan, false, &out.kernNext));
        // (the pools' layout is the later launches' form's: history-coded for PLAIN, and for no other)
        if ((plan.prm.histBits != 0) != ((bounce_form(false, plan.dof, plan.many, plan.sweptCubes, plan.mesh, plan.grouped, plan.tex, plan.bump, plan.plain) & kbPlain) != 0))
            return fail(PT_ERR_INVALID, "pt_init: internal error: history bits %d and the later bounces' form disagree", plan.prm.histBits);
        return PT_OK;
    };
    Planned step0;
    std::vector<Planned> later((size_t)steps - 1);
    if (steps > 1) {
        if (ngeoms > 0 && !geoms) return fail(PT_ERR_INVALID, "pt_init: null argument");
        for (int s = 1; s < steps; ++s)
            for (int g = 0; g < ngeoms; ++g) {
                const PtGeom &a = geoms[g], &b = geoms[(size_t)s * ngeoms + g];
                if (a.type != b.type || a.materialid != b.materialid)
                    return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_MOTION step %d: geom %d has another type or materialid than in step 0", s, g);
            }
        for (int s = 0; s < steps; ++s) {
            Planned &pl = s ? later[(size_t)s - 1] : step0;
            if (const int rc = plan_step(geoms + (size_t)s * (ngeoms > 0 ? ngeoms : 0), pl))
                return fail(rc, "pt_init: PT_FLAG_MOTION step %d: %s", s, std::string(g_err).c_str());
            if (!s) continue;
            if (const char *why = slots_mismatch(pl.plan, step0.plan))
                return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_MOTION step %d: its plan and step 0's differ in what the in-flight batches share: %s", s, why);
            if (!same_bytes(pl.plan.texels, step0.plan.texels) || !same_bytes(pl.plan.meshRecs, step0.plan.meshRecs))
                return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_MOTION step %d: internal error: its texels or mesh records are not step 0's", s);
        }
    } else {
        PTCHECK(plan_step(geoms, step0));
    }
    deviceGuard.armed = false;      // (planned: from here on the call's device is set as it always was)
    faceStream.release(); facePix.release(); faceBytes.release();
    ScenePlan &plan = step0.plan;
    const void *const kernFirst = step0.kernFirst, *const kernNext = step0.kernNext;
    if (steps > 1 && !invariant_tables_are_the_exchanged_ones(R().tab, plan))
        return fail(PT_ERR_INVALID, "pt_init: internal error: the tables PT_FLAG_MOTION holds once are not the camera-invariant ones");
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "pt_init: no HIP device (this library has no CPU fallback)");
    register_exit_handler();
    phase_end(0);      // host planning
    // PT_FLAG_TEMPORAL on the renderer that goes and on the one that comes, the same frame size and device: the context's history lives on,
    // and the old view -- if it committed anything -- is blended into it first, on the old renderer's stream (free_renderer waits for it)
    // (PT_FLAG_DEMOD_HISTORY: only between two renderers that agree on it -- a history with albedo and one without are different things)
    // (PT_FLAG_OBJECT_HISTORY: likewise only between two renderers that agree on it -- and between two that carry it only where the old and
    // the new scene describe the same objects, their poses aside: the caller's promise as a check)
    bool keepHistory = R().init && (R().flags & plan.flags & PT_FLAG_TEMPORAL) &&
                       !((R().flags ^ plan.flags) & (PT_FLAG_DEMOD_HISTORY | PT_FLAG_OBJECT_HISTORY)) &&
                       R().prm.W == plan.prm.W && R().prm.H == plan.prm.H && (o.device < 0 || o.device == R().device);
    const bool objectHistory = (plan.flags & PT_FLAG_OBJECT_HISTORY) != 0;
    if (keepHistory && objectHistory && !same_objects(R(), geoms, ngeoms, mats, nmats, reg)) keepHistory = false;
    PTCHECK(retire_view(keepHistory, "pt_init"));
    free_renderer(keepHistory);
    phase_end(1);      // the capture of history, the drain and the free

    State &S = R();
    static_cast<PlanScalars &>(S) = plan;
    S.kernFirst = kernFirst;
    S.kernNext = kernNext;
    if (o.device >= 0) HIPCHECK(hipSetDevice(o.device));
    HIPCHECK(hipGetDevice(&S.device));
    S.stream = (hipStream_t)o.stream;
    PTCHECK(refresh_motion(S.hist, objectHistory, geoms, ngeoms));      // (the capture, where one was due, is behind us)
    PTCHECK(S.hostFault.alloc(1, hipHostMallocMapped));
    *S.hostFault = 0u;
    HIPCHECK(hipHostGetDevicePointer((void **)&S.hostFaultDev, S.hostFault, 0));

    if (o.accum_dev) {
        S.image = o.accum_dev;
    } else {
        const size_t n = (S.flags & PT_FLAG_ACCUM_SHARD_ROWS) ? (size_t)(S.nLocal > 0 ? S.nLocal : 1) : (size_t)S.P;
        PTCHECK(S.imageOwn.alloc(n * 3));
        S.image = S.imageOwn.p;
        HIPCHECK(hipMemsetAsync(S.image, 0, n * 3 * sizeof(float), S.stream));
    }
    if (S.flags & PT_FLAG_MOMENTS) PTCHECK(S.moments.alloc_zeroed((size_t)S.P));
    // radiance buffers and iteration masks: the frame's pixels, or only this shard's (KParams::contribLocal)
    const size_t cpx = S.prm.contribLocal ? (size_t)(S.nLocal > 0 ? S.nLocal : 1) : (size_t)S.P;
    const size_t contribFloats = (size_t)S.maxBatch * cpx * 3, maskWords = (size_t)((S.maxBatch + 31) / 32) * cpx;
    {   // the memory budget BEFORE the first large allocation: a batch that does not fit fails here, with nothing to undo
        const size_t perSlot = 2 * (S.poolCap * poolDwords(S.prm.histBits) * sizeof(float) + (size_t)kSeg * S.poolChunks * sizeof(unsigned long long)) + sizeof(Ctrl) +
                               contribFloats * sizeof(float) + maskWords * sizeof(uint32_t) + S.meshHitWords * sizeof(unsigned long long);
        // ... and PT_FLAG_DISPLAY_FILTER's buffers: the guide buffers, the two float4 images of the levels, the bytes pt_readback_rgba8 copies
        const size_t display = (S.flags & PT_FLAG_DISPLAY_FILTER) ? (size_t)S.P * (4 * sizeof(float4) + sizeof(uchar4)) : 0;
        // ... and PT_FLAG_SPATIAL_VARIANCE's one image, the counts
        const size_t spatial = (S.flags & PT_FLAG_SPATIAL_VARIANCE) ? (size_t)S.P * sizeof(float) : 0;
        // ... and PT_FLAG_DEMODULATE's one image, the albedo sums
        const size_t albedo = (S.flags & PT_FLAG_DEMODULATE) ? (size_t)S.P * sizeof(float4) : 0;
        // ... and PT_FLAG_DEMOD_HISTORY's one image, the blended albedo
        const size_t albedoBlend = (S.flags & PT_FLAG_DEMOD_HISTORY) ? (size_t)S.P * sizeof(float4) : 0;
        // ... and PT_FLAG_MOTION's tables: every step's own, and the ones no pose changes once
        size_t poseTables = 0;
        if (steps > 1) {
            poseTables = table_bytes(plan, true) + table_bytes(plan, false);
            for (Planned &pl : later) poseTables += table_bytes(pl.plan, false);
        }
        const size_t need = perSlot * (size_t)S.nslots + display + spatial + albedo + albedoBlend + poseTables;
        size_t freeB = 0, totalB = 0;
        HIPCHECK(hipMemGetInfo(&freeB, &totalB));
        if (need > freeB)
            return fail(PT_ERR_HIP, "pt_init: %.2f GB of path pools and radiance buffers (max_batch %d x pipeline_depth %d) exceed the %.2f GB of free "
                        "device memory: lower max_batch or pipeline_depth", need / 1e9, S.maxBatch, S.nslots, freeB / 1e9);
    }
    if (S.flags & PT_FLAG_DISPLAY_FILTER) {      // (pt_iterate under the flag allocates nothing)
        PTCHECK(S.dnPosT.alloc((size_t)S.P));
        PTCHECK(S.dnNrmId.alloc((size_t)S.P));
        for (auto &ping : S.dnPing) PTCHECK(ping.alloc((size_t)S.P));
        PTCHECK(S.dnRgba.alloc((size_t)S.P));
    }
    if (S.flags & PT_FLAG_SPATIAL_VARIANCE) PTCHECK(S.dnCount.alloc((size_t)S.P));
    if (S.flags & PT_FLAG_DEMODULATE) PTCHECK(S.albedo.alloc_zeroed((size_t)S.P));
    if (S.flags & PT_FLAG_DEMOD_HISTORY) PTCHECK(S.dnAlbedo.alloc((size_t)S.P));
    for (int i = 0; i < S.nslots; ++i) {
        Slot &sl = S.slot[i];
        PTCHECK(sl.stream.create(hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            PTCHECK(sl.pathbuf[b].alloc(S.poolCap * poolDwords(S.prm.histBits)));
            PTCHECK(sl.chunkList[b].alloc_zeroed((size_t)kSeg * S.poolChunks));
        }
        PTCHECK(sl.ctrl.alloc(1));
        PTCHECK(reset_ctrl(sl.ctrl.p, nullptr));
        PTCHECK(sl.contrib.alloc_zeroed(contribFloats));
        PTCHECK(sl.hitMask.alloc_zeroed(maskWords));
        if (S.meshHitWords) PTCHECK(sl.meshHit.alloc(S.meshHitWords));
        PTCHECK(sl.evDone.create(hipEventDisableTiming));
        PTCHECK(sl.evCommitted.create(hipEventDisableTiming));
    }

    // the plan's tables, each once; a table the scene does not have is empty and stays without a buffer (the walks' tables of a scene with
    // meshes and the groups of a grouped one get theirs even when empty: a kernel may be handed the pointer of an empty table)
    phase_end(2);      // streams, events and every allocation with its zeroing
    PTCHECK(S.tab.for_each(nullptr, plan, S.mesh, S.grouped, [](auto &buf, const auto *, const auto &table, TableRule rule) {
        return rule.allocated(table.size()) ? buf.upload(table.data(), table.size(), rule.slack) : (int)PT_OK;
    }));

    // PT_FLAG_MOTION: the later steps' poses -- scalars, kernels, tables (but the ones step 0's upload holds for all), each sized like step 0
    if (steps > 1) {
        S.poses.resize((size_t)steps);
        S.step = 0;
        for (int s = 1; s < steps; ++s) {
            Planned &pl = later[(size_t)s - 1];
            Pose &p = S.poses[(size_t)s];
            p.scalars = pl.plan;
            p.kernFirst = pl.kernFirst;
            p.kernNext = pl.kernNext;
            PTCHECK(p.tab.for_each(nullptr, pl.plan, pl.plan.mesh, pl.plan.grouped, [](auto &buf, const auto *, const auto &table, TableRule rule) {
                return !rule.cameraInvariant && rule.allocated(table.size()) ? buf.upload(table.data(), table.size(), rule.slack) : (int)PT_OK;
            }));
        }
    }
    S.tables = State::TableCount();
    S.tables.ownBytes = (long long)table_bytes(plan, false, &S.tables.ownBuffers);
    S.tables.sharedBytes = (long long)table_bytes(plan, true, &S.tables.sharedBuffers);
    S.tables.allOwnBytes = S.tables.ownBytes;
    for (Planned &pl : later) S.tables.allOwnBytes += (long long)table_bytes(pl.plan, false);
    phase_end(3);      // the tables' uploads
    for (int s = steps - 1; s >= 0; --s) {      // (step 0 last: the pose the renderer starts in)
        activate_step(S, s);
        PTCHECK(size_launches(S));
    }
    PTCHECK(lds_attributes(S));
    const KParams &k = S.prm;
    if (env_flag("PT_AMD_VERBOSE"))       // experiments: what pt_init decided
        fprintf(stderr, "pt_init: lds %zu / %zu B, grid %d / %d, mesh %d many %d plain %d, binned %d walls %d (slots %d, planes %d) allClassified %d, sphCull %d (cluster 0: %d) omax %g\n",
                S.ldsBytes, S.ldsBytesNext, S.gridFirst, S.grid, (int)S.mesh, (int)S.many, (int)S.plain, k.nBinned, k.nWalls, k.nSlotWalls, k.nPlaneWalls, k.allClassified, k.nSphCull,
                k.sphN0, (double)k.sphOMax);
    HIPCHECK(hipDeviceSynchronize());
    phase_end(4);      // launch sizing and the final synchronise
    if (phases)
        fprintf(stderr, "pt_init phases ms: plan %.3f free %.3f allocate %.3f upload %.3f size+sync %.3f\n", phaseMs[0], phaseMs[1], phaseMs[2], phaseMs[3], phaseMs[4]);
    // what the camera move needs of this call: its scene arguments, and the plan whose tables the device now holds
    // (PT_FLAG_MOTION: every step's geoms -- its move is the full call --, and no held plan)
    S.inGeoms.assign(geoms, geoms + (size_t)steps * ngeoms);
    S.inMats.assign(mats, mats + nmats);
    S.inDepth = traceDepth;
    S.inOpts = o;
    S.initReg = reg;
    if (steps == 1) {
        drop_camera_invariant(S.tab, plan);
        S.held.reset(new ScenePlan(std::move(plan)));
    }
    S.init = true;
    g_err.clear();
    return PT_OK;
}

// ---- the camera move ------------------------------------------------------------------------------------------------------------------------
// which way the calling thread's last camera move went (pt_test_last_camera_move): fast 1 / 0, -1 before the first move or after a
// refusal; the tables and bytes the fast path uploaded
struct CameraMove { int fast = -1, tables = 0; long long bytes = 0; };
thread_local CameraMove t_lastMove;
// PT_FLAG_KEEP_RENDERER: why the calling thread's last flagged full call did not take the move's path (keep_renderer_mismatch's answer, or
// that there was no renderer; null: it did, or there has been no such call)
thread_local const char *t_keepWhy = nullptr;

// The work list's face certificates on the device, between build_camera_list's two passes: the pixel words of the one-cube groups whose
// cube is CubeCert::ok go up as one array, k_camera_faces runs once per group -- the cube is uniform per group: a kernel argument -- and
// the bytes come back as CameraGroups::faces.  pix / face: scratch buffers of the caller's, grown where needed; ms (or NULL): the kernels'
// time by HIP events.
int camera_faces_device(CameraGroups &G, const CameraResolve &cr, hipStream_t st, DevBuf<uint32_t> &pix, DevBuf<signed char> &face, float *ms) {
    if (ms) *ms = 0.0f;
    struct Run { size_t group, off, n; int cube; };
    std::vector<Run> runs;
    size_t total = 0;
    for (size_t s = 0; s < G.groups.size(); ++s) {
        const int cube = camera_group_cube(G, s, cr);
        if (cube < 0 || G.groups[s].empty()) continue;
        runs.push_back({s, total, G.groups[s].size(), cube});
        total += G.groups[s].size();
    }
    if (!total) return PT_OK;
    std::vector<uint32_t> words(total);
    for (const Run &r : runs) memcpy(words.data() + r.off, G.groups[r.group].data(), r.n * sizeof(uint32_t));
    if (pix.cap < total) PTCHECK(pix.alloc(total + total / 4));
    if (face.cap < total) PTCHECK(face.alloc(total + total / 4));
    Event ev[2];
    HIPCHECK(hipMemcpyAsync(pix.p, words.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (ms) {
        for (Event &e : ev) PTCHECK(e.create(hipEventDefault));
        HIPCHECK(hipEventRecord(ev[0], st));
    }
    for (const Run &r : runs) {
        CameraFacesArgs A;
        A.cube = cr.cube[(size_t)r.cube];
        A.basis = cr;
        A.pix = pix.p + r.off;
        A.face = face.p + r.off;
        A.n = (int)r.n;
        hipLaunchKernelGGL(k_camera_faces, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, st, A);
    }
    HIPCHECK(hipGetLastError());
    if (ms) HIPCHECK(hipEventRecord(ev[1], st));
    std::vector<signed char> bytes(total);
    HIPCHECK(hipMemcpyAsync(bytes.data(), face.p, total, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (ms) HIPCHECK(hipEventElapsedTime(ms, ev[0], ev[1]));
    for (const Run &r : runs) {
        std::vector<int> &f = G.faces[r.group];
        f.resize(r.n);
        for (size_t i = 0; i < r.n; ++i) {
            const int v = bytes[r.off + i];
            if (v < -1 || v > 5) return fail(PT_ERR_DEVICE, "pt_init (camera move): k_camera_faces answered %d", v);
            f[i] = v;
        }
    }
    return PT_OK;
}

// The camera move's action on a table (SceneTables::for_each): the renderer's against the new plan's -- left alone where the device holds
// these very bytes (a camera-invariant one: always), released where the plan has none (pt_init leaves such a table without a buffer, and
// the kernels ask), written in place where it fits, reallocated where it grew.  The copy is enqueued on `st` from `now`, which the caller
// keeps until the stream has been waited for.
template <typename T>
int refresh_table(DevBuf<T> &buf, const std::vector<T> &heldT, const std::vector<T> &now, TableRule rule, hipStream_t st, CameraMove &mv) {
    if (rule.cameraInvariant) return PT_OK;
    if (now.empty() && !rule.evenEmpty) { buf.release(); return PT_OK; }
    const bool same = buf.p && heldT.size() == now.size() && (now.empty() || !memcmp(heldT.data(), now.data(), now.size() * sizeof(T)));
    if (same) return PT_OK;
    if (!buf.p || buf.cap < now.size()) PTCHECK(buf.alloc(now.size() + now.size() / 4));
    if (!now.empty()) HIPCHECK(hipMemcpyAsync(buf.p, now.data(), now.size() * sizeof(T), hipMemcpyHostToDevice, st));
    mv.tables += 1;
    mv.bytes += (long long)(now.size() * sizeof(T));
    return PT_OK;
}

// pt_init over the live renderer with the scene it was initialised with -- its arguments, and what was registered then --: the camera
// move's slow path.  What has been registered since stays registered behind it.  (Copies: init_renderer frees the renderer that holds them.)
int reinit_with_camera(const PtCamera &cam) {
    State &S = R();
    const std::vector<PtGeom> geoms = S.inGeoms;
    const std::vector<PtMaterial> mats = S.inMats;
    const PtOptions o = S.inOpts;
    Stream camStream = std::move(S.camStream);      // (the moves' own stream outlives a rebuild -- not one that fails and leaves a State that holds nothing)
    const int ngeoms = (int)(geoms.size() / ((o.flags & PT_FLAG_MOTION) ? PT_MOTION_STEPS : 1));      // (PT_FLAG_MOTION: every step's geoms)
    const int rc = init_renderer(&cam, geoms.data(), ngeoms, mats.data(), (int)mats.size(), S.inDepth, o, S.initReg);
    if (!S.holds_nothing()) S.camStream = std::move(camStream);
    return rc;
}

// PT_FLAG_KEEP_RENDERER on a full call: the call against the live renderer's copies of its own (pt_scene_plan.h: keep_renderer_mismatch).
// What is registered now and what the renderer was initialised with share every part no pt_set_* call has replaced in between.
const char *keep_mismatch(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions &o) {
    const State &S = R();
    if (!S.init) return "no live renderer";
    if (!cam) return "camera";
    const InitCall now{geoms, ngeoms, mats, nmats, traceDepth, &o, cam->resolution[0], cam->resolution[1], S.reg};
    const InitCall then{S.inGeoms.data(), (int)S.inGeoms.size(), S.inMats.data(), (int)S.inMats.size(), S.inDepth, &S.inOpts, S.prm.W, S.prm.H, S.initReg};
    return keep_renderer_mismatch(now, then);
}

int set_camera(const PtCamera *cam) {
    t_lastMove = CameraMove();
    if (!cam) return fail(PT_ERR_INVALID, "pt_init (camera move): null camera");
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_init (camera move) before pt_init: there is no renderer whose scene it could name");
    State &S = R();
    if (cam->resolution[0] != S.prm.W || cam->resolution[1] != S.prm.H)
        return fail(PT_ERR_INVALID, "pt_init (camera move): the camera's resolution %d x %d is not the renderer's %d x %d (pt_init makes a renderer of another size)",
                    cam->resolution[0], cam->resolution[1], S.prm.W, S.prm.H);
    const PtCamera camNew = *cam;        // (the caller may hand in the camera of a scene this call outlives)
    if (S.device >= 0) HIPCHECK(hipSetDevice(S.device));
    // PT_FLAG_MOTION: the full call with all of the renderer's steps, which plans them before it touches anything
    if (S.flags & PT_FLAG_MOTION) {
        t_lastMove.fast = 0;
        return reinit_with_camera(camNew);
    }
    // 1. the plan for the new camera, the certificates of its work list on the device; a scene that is refused has touched nothing
    if (!S.camStream) PTCHECK(S.camStream.create(hipStreamNonBlocking));
    std::unique_ptr<ScenePlan> planPtr(new ScenePlan);
    ScenePlan &plan = *planPtr;
    {
        SceneIn in(&camNew, S.inGeoms.data(), (int)S.inGeoms.size(), S.inMats.data(), (int)S.inMats.size(), S.inDepth, S.inOpts, S.initReg);
        in.faces = [&S](CameraGroups &G, const CameraResolve &cr) { return camera_faces_device(G, cr, S.camStream, S.camPixScratch, S.camFaceScratch, nullptr); };
        PTCHECK(plan_scene(in, plan));
    }
    const void *kernFirst = nullptr, *kernNext = nullptr;
    PTCHECK(resolve_bounce_kernel(plan, true, &kernFirst));
    PTCHECK(resolve_bounce_kernel(plan, false, &kernNext));
    // 2. drain the renderer's streams, as free_renderer does
    for (int i = 0; i < S.nslots; ++i) (void)hipStreamSynchronize(S.slot[i].stream);
    (void)hipStreamSynchronize(S.stream);
    // 3. does the plan need the allocations the renderer holds?  (It does unless planning changes: none of these sizes depends on the
    // camera; a camera-invariant table's buffer is the one pt_init would make for the plan's.)  A renderer that carries a sticky device
    // fault is rebuilt like any other: pt_init.
    const bool faulted = S.hostFault && *(volatile uint32_t *)S.hostFault != 0u;
    bool sameInvariants = true;
    (void)S.tab.for_each(S.held.get(), plan, plan.mesh, plan.grouped, [&](const auto &buf, const auto *, const auto &now, TableRule rule) {
        if (rule.cameraInvariant && buf.cap != rule.allocated(now.size())) sameInvariants = false;
        return (int)PT_OK;
    });
    const bool sameAllocations = S.held && kernFirst == S.kernFirst && kernNext == S.kernNext && !slots_mismatch(plan, S) && sameInvariants;
    if (faulted || !sameAllocations) {
        t_lastMove.fast = 0;
        return reinit_with_camera(camNew);
    }
    // batches traced ahead are discarded: consumed without being added, which leaves the slots' iteration masks zeroed
    // (A HIP call that fails up to the capture has overwritten nothing the full call needs: the full call is made instead.)
    const auto slow = [&]() { t_lastMove.fast = 0; return reinit_with_camera(camNew); };
    if (!S.ahead.empty() && (discard_ahead() != PT_OK || hipStreamSynchronize(S.stream) != hipSuccess)) return slow();
    // 5. the old view becomes the context's history exactly as pt_init captures it -- or the history ends as it ends there
    {
        bool keepHistory = (S.flags & PT_FLAG_TEMPORAL) != 0;
        // (PT_FLAG_DISPLAY_FILTER, whose pt_iterate allocates nothing: the capture exchanges the renderer's guide buffers with the
        // history's, so a history that has none yet is given a pair first)
        if (capture_due(keepHistory) && (S.flags & PT_FLAG_DISPLAY_FILTER) && !S.hist.hpos.p && !S.hist.live &&
            (S.hist.hpos.alloc((size_t)S.P) != PT_OK || S.hist.hnrm.alloc((size_t)S.P) != PT_OK)) {
            S.hist.hpos.release(); S.hist.hnrm.release();
            return slow();
        }
        PTCHECK(retire_view(keepHistory, "pt_init (camera move)"));
        if (!keepHistory) S.hist = History();
        // (PT_FLAG_OBJECT_HISTORY: the same scene in the poses just captured -- no table; a history no capture was due for keeps its poses)
        PTCHECK(refresh_motion(S.hist, (S.flags & PT_FLAG_OBJECT_HISTORY) != 0, S.inGeoms.data(), (int)S.inGeoms.size()));
    }
    // From here on the renderer is overwritten: a HIP call that fails leaves the context without a renderer, as pt_init's do.
    const auto body = [&]() -> int {
        // 6. the library's accumulators, on the renderer's stream (a caller-owned accum_dev stays the caller's to zero)
        if (S.imageOwn.p) HIPCHECK(hipMemsetAsync(S.imageOwn.p, 0, S.imageOwn.cap * sizeof(float), S.stream));
        if (S.moments.p) HIPCHECK(hipMemsetAsync(S.moments.p, 0, (size_t)S.P * sizeof(float), S.stream));
        if (S.albedo.p) HIPCHECK(hipMemsetAsync(S.albedo.p, 0, (size_t)S.P * sizeof(float4), S.stream));
        // 7. the slots' counters (the chunk lists' generations go on: an entry of the old view never carries a serial number to come), and the
        // host's sequence, trace-ahead, guide and timing state
        for (int i = 0; i < S.nslots; ++i) {
            HIPCHECK(hipMemsetAsync(S.slot[i].ctrl.p, 0, sizeof(Ctrl), S.stream));
            S.slot[i].parity = 0;
        }
        recycle_events(S.evBounce);
        S.msBounce = 0; S.nBounce = 0;
        S.iterations = 0; S.committed = 0; S.seq = 0;
        S.ahead.clear();
        S.dnGuideIter = 0;
        S.snapTarget = nullptr; S.snapWait = nullptr;
        // 8. the new plan's scalars
        static_cast<PlanScalars &>(S) = plan;
        S.kernFirst = kernFirst;
        S.kernNext = kernNext;
        // 9. the tables whose bytes differ (textures and mesh records: never -- no camera changes them, and the plan is the same scene's)
        CameraMove &mv = t_lastMove;
        PTCHECK(S.tab.for_each(S.held.get(), plan, S.mesh, S.grouped, [&](auto &buf, const auto *heldT, const auto &now, TableRule rule) {
            return refresh_table(buf, *heldT, now, rule, S.stream, mv);
        }));
        // 10. what depends on the tables: the LDS attributes, the grids, the packed list or the row bands
        PTCHECK(size_launches(S));
        // the copies read the plan's vectors and the slots' streams do not wait for the renderer's: everything above has landed before
        // the next launch is enqueued
        HIPCHECK(hipStreamSynchronize(S.stream));
        return PT_OK;
    };
    const int rc = body();
    if (rc) {
        const std::string err = g_err;
        free_renderer();
        g_err = err;
        t_lastMove = CameraMove();
        return rc;
    }
    drop_camera_invariant(S.tab, plan);
    S.held = std::move(planPtr);
    t_lastMove.fast = 1;
    g_err.clear();
    return PT_OK;
}

// What pt_iterate_batch does for iterations first_iter .. first_iter + count - 1, its checks behind it: the next slot, trace, wait, commit in
// order -- for a whole call, or under PT_FLAG_MOTION for each piece of it that lies in one run, which sees one pose.  single: the CALL is
// one iteration (a piece of one iteration cut from a longer call is no reason to trace ahead).
int iterate_piece(int first_iter, int count, bool single) {
    int rc;
    if ((R().flags & PT_FLAG_TRACE_AHEAD) && single) {
        // the reference's protocol, one call per iteration: the iteration comes out of a batch that was traced ahead
        if (!R().ahead.empty() && R().ahead.front().first + R().ahead.front().next != first_iter) {
            rc = discard_ahead();                    // not the iteration the parked batches continue with
            if (rc) return rc;
        }
        if (R().ahead.empty()) {
            rc = trace_ahead(first_iter);
            if (rc) return rc;
        }
        State::Parked &p = R().ahead.front();
        Slot &sl = R().slot[p.slot];
        if (!p.waited) {      // (once per batch: the commits that follow on the caller's stream are ordered behind this one)
            HIPCHECK(hipStreamWaitEvent(R().stream, sl.evDone, 0));
            p.waited = true;
        }
        rc = commit_range(sl, p.count, p.next, p.next + 1, false);
        if (rc) return rc;
        int after = p.first + p.count;               // first iteration behind the parked batches
        if (++p.next == p.count) {
            HIPCHECK(hipEventRecord(sl.evCommitted, R().stream));
            R().ahead.pop_front();
        }
        // every free slot traces on: the GPU stays ahead of the caller by at least a batch
        if (!R().ahead.empty()) after = R().ahead.back().first + R().ahead.back().count;
        while ((int)R().ahead.size() < R().nslots && after < kIterEnd) {
            rc = trace_ahead(after);
            if (rc) return rc;
            after = R().ahead.back().first + R().ahead.back().count;
        }
    } else {
        if (!R().ahead.empty()) {
            rc = discard_ahead();
            if (rc) return rc;
        }
        activate_step(R(), motion_step(first_iter));      // (PT_FLAG_MOTION: the piece's pose; else nothing)
        Slot &sl = R().slot[R().seq % R().nslots];
        rc = trace_batch(sl, first_iter, count);
        if (rc) return rc;
        // commit on the caller's stream: commits are therefore ordered like the pt_iterate calls
        HIPCHECK(hipStreamWaitEvent(R().stream, sl.evDone, 0));
        rc = commit_range(sl, count, 0, count, false);
        if (rc) return rc;
        HIPCHECK(hipEventRecord(sl.evCommitted, R().stream));
        R().seq += 1;
    }
    return PT_OK;
}

}  // namespace
#pragma GCC visibility push(default)
extern "C" {

int pt_set_meshes_sized(const PtMesh *meshes, int nmeshes, size_t mesh_struct_bytes) {
    if (mesh_struct_bytes != sizeof(PtMesh))
        return fail(PT_ERR_INVALID, "pt_set_meshes: the caller's PtMesh is %zu bytes, this library's %zu (built against another pt_amd.h: ABI version %d here)",
                    mesh_struct_bytes, sizeof(PtMesh), PT_AMD_ABI_VERSION);
    return pt_set_meshes(meshes, nmeshes);
}

int pt_set_meshes(const PtMesh *meshes, int nmeshes) {
    if (nmeshes < 0 || (nmeshes && !meshes)) return fail(PT_ERR_INVALID, "pt_set_meshes: null argument");
    for (int i = 0; i < nmeshes; ++i) {
        if (meshes[i].geom < 0 || meshes[i].ntris < 1 || !meshes[i].tris) return fail(PT_ERR_INVALID, "pt_set_meshes: mesh %d is empty", i);
        for (int j = 0; j < i; ++j)
            if (meshes[j].geom == meshes[i].geom) return fail(PT_ERR_INVALID, "pt_set_meshes: geom %d given twice", meshes[i].geom);
        for (size_t q = 0; q < 9 * (size_t)meshes[i].ntris; ++q)
            if (!std::isfinite(meshes[i].tris[q])) return fail(PT_ERR_INVALID, "pt_set_meshes: mesh %d holds a non-finite coordinate", i);
        if (meshes[i].normals)
            for (size_t q = 0; q < 9 * (size_t)meshes[i].ntris; ++q)
                if (!std::isfinite(meshes[i].normals[q])) return fail(PT_ERR_INVALID, "pt_set_meshes: mesh %d holds a non-finite normal", i);
    }
    std::vector<ptm::HostMesh> reg;
    for (int i = 0; i < nmeshes; ++i) {
        ptm::HostMesh m;
        m.geom = meshes[i].geom;
        m.tris.assign(meshes[i].tris, meshes[i].tris + 9 * (size_t)meshes[i].ntris);
        if (meshes[i].normals) m.normals.assign(meshes[i].normals, meshes[i].normals + 9 * (size_t)meshes[i].ntris);
        if (meshes[i].materials) m.mats.assign(meshes[i].materials, meshes[i].materials + (size_t)meshes[i].ntris);
        reg.push_back(std::move(m));
    }
    R().reg.meshes = std::make_shared<const std::vector<ptm::HostMesh>>(std::move(reg));      // (a live renderer keeps the part it was initialised with)
    return PT_OK;
}

int pt_set_bump_maps(const PtBumpBinding *bindings, int nbindings, size_t binding_struct_bytes) {
    if (binding_struct_bytes != sizeof(PtBumpBinding))
        return fail(PT_ERR_INVALID, "pt_set_bump_maps: the caller's PtBumpBinding is %zu bytes, this library's %zu (ABI version %d here)",
                    binding_struct_bytes, sizeof(PtBumpBinding), PT_AMD_ABI_VERSION);
    if (nbindings < 0 || (nbindings && !bindings)) return fail(PT_ERR_INVALID, "pt_set_bump_maps: null argument");
    for (int i = 0; i < nbindings; ++i)
        if (bindings[i].ntris < 0 || (bindings[i].ntris > 0 && !bindings[i].uvs)) return fail(PT_ERR_INVALID, "pt_set_bump_maps: binding %d: bad UVs", i);
    // (indices, counts and the scale are checked by pt_init, against the scene)
    std::vector<HostBumpBinding> reg;
    for (int i = 0; i < nbindings; ++i) {
        HostBumpBinding b;
        b.geom = bindings[i].geom; b.texture = bindings[i].texture; b.ntris = bindings[i].ntris; b.scale = bindings[i].scale;
        if (bindings[i].uvs) b.uvs.assign(bindings[i].uvs, bindings[i].uvs + 6 * (size_t)b.ntris);
        reg.push_back(std::move(b));
    }
    R().reg.bumpBindings = std::make_shared<const std::vector<HostBumpBinding>>(std::move(reg));
    return PT_OK;
}

int pt_set_textures(const PtTexture *textures, int ntextures, size_t texture_struct_bytes, const PtTexBinding *bindings, int nbindings,
                    size_t binding_struct_bytes) {
    if (texture_struct_bytes != sizeof(PtTexture) || binding_struct_bytes != sizeof(PtTexBinding))
        return fail(PT_ERR_INVALID, "pt_set_textures: the caller's PtTexture / PtTexBinding are %zu / %zu bytes, this library's %zu / %zu (ABI version %d here)",
                    texture_struct_bytes, binding_struct_bytes, sizeof(PtTexture), sizeof(PtTexBinding), PT_AMD_ABI_VERSION);
    if (ntextures < 0 || nbindings < 0 || (ntextures && !textures) || (nbindings && !bindings)) return fail(PT_ERR_INVALID, "pt_set_textures: null argument");
    // (sizes, indices and values are checked by pt_init, against the scene; what cannot be copied safely is not copied and refused there)
    for (int i = 0; i < ntextures; ++i)
        if (textures[i].width >= 1 && textures[i].width <= kTexSizeMax && textures[i].height >= 1 && textures[i].height <= kTexSizeMax && !textures[i].rgb)
            return fail(PT_ERR_INVALID, "pt_set_textures: texture %d has no texels", i);
    for (int i = 0; i < nbindings; ++i)
        if (bindings[i].ntris < 0 || (bindings[i].ntris > 0 && !bindings[i].uvs)) return fail(PT_ERR_INVALID, "pt_set_textures: binding %d: bad UVs", i);
    std::vector<HostTexture> regTex;
    std::vector<HostTexBinding> regBind;
    long long texels = 0;
    for (int i = 0; i < ntextures; ++i) {
        HostTexture t;
        t.w = textures[i].width; t.h = textures[i].height;
        const bool sized = t.w >= 1 && t.w <= kTexSizeMax && t.h >= 1 && t.h <= kTexSizeMax;
        if (sized) texels += (long long)t.w * t.h;
        if (sized && texels < kTexTexelsMax) t.rgb.assign(textures[i].rgb, textures[i].rgb + (size_t)t.w * t.h * 3);
        regTex.push_back(std::move(t));
    }
    for (int i = 0; i < nbindings; ++i) {
        HostTexBinding b;
        b.geom = bindings[i].geom; b.texture = bindings[i].texture; b.ntris = bindings[i].ntris;
        if (bindings[i].uvs) b.uvs.assign(bindings[i].uvs, bindings[i].uvs + 6 * (size_t)b.ntris);
        regBind.push_back(std::move(b));
    }
    R().reg.textures = std::make_shared<const std::vector<HostTexture>>(std::move(regTex));
    R().reg.texBindings = std::make_shared<const std::vector<HostTexBinding>>(std::move(regBind));
    return PT_OK;
}

// pt_init's three forms: the camera move (no scene at all and PT_SAME_SCENE for the depth name the scene the live renderer was initialised
// with), the full call that PT_FLAG_KEEP_RENDERER finds to be the live renderer's own with another pose -- the camera move too --, and the
// full call (init_renderer, with what is registered now).
int pt_init(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth,
            const PtOptions *opts) {
    if (!geoms && !mats && ngeoms == 0 && nmats == 0 && traceDepth == PT_SAME_SCENE && !opts) return set_camera(cam);
    const PtOptions o = effective_options(opts);
    if (o.flags & PT_FLAG_KEEP_RENDERER) {
        t_lastMove = CameraMove();
        t_keepWhy = keep_mismatch(cam, geoms, ngeoms, mats, nmats, traceDepth, o);
        if (!t_keepWhy) {
            R().initReg = R().reg;      // (equal registrations: the renderer's own copies of what a pt_set_* call has replaced with the same bytes are let go)
            return set_camera(cam);
        }
    }
    return init_renderer(cam, geoms, ngeoms, mats, nmats, traceDepth, o, R().reg);
}

int pt_iterate_batch(int frame, int first_iter, int count, void *rgba8_dev) {
    (void)frame;  // always 0 in the reference (src/main.cpp:102)
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_iterate before pt_init");
    if (count < 1 || count > R().maxBatch) return fail(PT_ERR_INVALID, "pt_iterate_batch: count must be 1..max_batch (%d)", R().maxBatch);
    if (first_iter < 1 || first_iter + count - 1 >= kIterEnd)
        return fail(PT_ERR_INVALID, "pt_iterate: iter must be 1..4194303 (seed bits, pathtrace.cu:43)");
    // every argument is checked BEFORE anything is enqueued: a rejected call leaves the image and the counters untouched
    if (rgba8_dev && (R().flags & PT_FLAG_ACCUM_SHARD_ROWS))
        return fail(PT_ERR_INVALID, "pt_iterate: no PBO conversion from a row-sharded accumulator");
    if (R().poses.empty()) {
        PTCHECK(iterate_piece(first_iter, count, count == 1));
    } else {      // PT_FLAG_MOTION: cut at the run boundaries; the PBO conversion happens once, after the last piece
        for (int i = first_iter, end = first_iter + count; i < end;) {
            const int n = std::min(end, motion_run_end(i)) - i;
            PTCHECK(iterate_piece(i, n, count == 1));
            i += n;
        }
    }
    // PT_FLAG_DEMODULATE: the albedo of the iterations just committed, behind the commit on the caller's stream (never with batches traced ahead)
    if (R().flags & PT_FLAG_DEMODULATE) PTCHECK(albedo_launch(first_iter, count));
    if (rgba8_dev && (R().flags & PT_FLAG_DISPLAY_FILTER)) {
        // the display filter: the guide buffers (once), the blend with the history, the levels, the bytes -- all behind the commit
        PTCHECK(display_bytes(first_iter + count - 1, reinterpret_cast<uchar4 *>(rgba8_dev), "pt_iterate"));
    } else if (rgba8_dev) {
        hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().image, R().P,
                           first_iter + count - 1, reinterpret_cast<uchar4 *>(rgba8_dev));
        HIPCHECK(hipGetLastError());
    }
    R().iterations += count;
    R().committed += count;
    return PT_OK;
}

int pt_iterate(int frame, int iter, void *rgba8_dev) { return pt_iterate_batch(frame, iter, 1, rgba8_dev); }

int pt_sync(void) {
    if (!R().init) {
        if (!scan_in_use()) return fail(PT_ERR_NOT_INIT, "pt_sync before pt_init");
        HIPCHECK(hipDeviceSynchronize());          // the scan library alone (the current device's calls)
        return PT_OK;
    }
    return check_device_fault();
}

int pt_readback(float *rgb_sum_host) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_readback before pt_init");
    if (!rgb_sum_host) return fail(PT_ERR_INVALID, "pt_readback: null");
    // every commit so far is already ordered before this copy on the caller's stream
    if (R().flags & PT_FLAG_ACCUM_SHARD_ROWS) {   // scatter this shard's rows into a zeroed full frame
        std::vector<float> rows((size_t)R().nLocal * 3);
        if (R().nLocal) HIPCHECK(hipMemcpyAsync(rows.data(), R().image, rows.size() * sizeof(float), hipMemcpyDeviceToHost, R().stream));
        HIPCHECK(hipStreamSynchronize(R().stream));
        memset(rgb_sum_host, 0, (size_t)R().P * 3 * sizeof(float));
        const size_t rowFloats = (size_t)R().prm.W * 3;
        for (int lr = 0; lr * R().prm.W < R().nLocal; ++lr)
            memcpy(rgb_sum_host + (size_t)(lr * R().prm.shardCount + R().prm.shardRank) * rowFloats, rows.data() + lr * rowFloats,
                   rowFloats * sizeof(float));
        return readback_fault();
    }
    // a plain copy: at PCIe rate into a buffer the caller has page-locked with pt_pin_host, through the runtime's
    // pageable staging path otherwise.  The library never registers memory it does not own on its own initiative.
    const size_t bytes = (size_t)R().P * 3 * sizeof(float);
    HIPCHECK(hipMemcpyAsync(rgb_sum_host, R().image, bytes, hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

int pt_pin_host(void *host, size_t bytes) {
    if (!host || bytes == 0) return fail(PT_ERR_INVALID, "pt_pin_host: bad argument");
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device");
    if (R().pinnedHost) {
        if (R().pinnedHost == host && R().pinnedBytes == bytes) return PT_OK;
        (void)hipHostUnregister(R().pinnedHost);
        R().pinnedHost = nullptr;
    }
    HIPCHECK(hipHostRegister(host, bytes, hipHostRegisterDefault));
    R().pinnedHost = host;
    R().pinnedBytes = bytes;
    return PT_OK;
}

int pt_unpin_host(void) {
    if (R().pinnedHost) {
        (void)hipStreamSynchronize(R().stream);
        HIPCHECK(hipHostUnregister(R().pinnedHost));
        R().pinnedHost = nullptr;
        R().pinnedBytes = 0;
    }
    return PT_OK;
}

int pt_readback_rgba8(int iter, uint8_t *rgba_host) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_readback_rgba8 before pt_init");
    if (!rgba_host || iter < 1) return fail(PT_ERR_INVALID, "pt_readback_rgba8: bad argument");
    if (R().flags & PT_FLAG_ACCUM_SHARD_ROWS) return fail(PT_ERR_INVALID, "pt_readback_rgba8: accumulator is row-sharded");
    if (R().flags & PT_FLAG_DISPLAY_FILTER) {
        PTCHECK(display_bytes(iter, R().dnRgba.p, "pt_readback_rgba8"));
        HIPCHECK(hipMemcpyAsync(rgba_host, R().dnRgba.p, (size_t)R().P * 4, hipMemcpyDeviceToHost, R().stream));
        HIPCHECK(hipStreamSynchronize(R().stream));
        return readback_fault();
    }
    DevBuf<uchar4> tmp;
    int rc = tmp.alloc(R().P);
    if (rc) return rc;
    hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().image, R().P, iter, tmp.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(rgba_host, tmp.p, (size_t)R().P * 4, hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

// ---- the denoiser: an edge-avoiding a-trous filter over the accumulator's mean (pt_denoise.h) -------------------------------
int pt_denoise(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, float *rgb_mean_host) {
    return denoise_to_host(samples, p, params_struct_bytes, kAtrousAuto, nullptr, rgb_mean_host, "pt_denoise");
}

int pt_denoise_rgba8(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, uint8_t *rgba_host) {
    if (!rgba_host) return fail(PT_ERR_INVALID, "pt_denoise_rgba8: null");
    int rc = denoise_run(samples, p, params_struct_bytes, kAtrousAuto, nullptr, "pt_denoise_rgba8");
    if (rc) return rc;
    if (!R().dnRgba.p) PTCHECK(R().dnRgba.alloc((size_t)R().P));
    // sendImageToPBO's conversion of the filtered MEAN: k_to_rgba8 with one sample (x / 1 is exact)
    hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().dnOut.p, R().P, 1, R().dnRgba.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(rgba_host, R().dnRgba.p, (size_t)R().P * 4, hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

// ---- the second moments (PT_FLAG_MOMENTS), the variance of the mean, and the filter it guides (pt_denoise.h) -------------------------
int pt_readback_moments(float *lum_sq_sum_host) {
    PTCHECK(moments_refusals("pt_readback_moments"));
    if (!lum_sq_sum_host) return fail(PT_ERR_INVALID, "pt_readback_moments: null");
    HIPCHECK(hipMemcpyAsync(lum_sq_sum_host, R().moments.p, (size_t)R().P * sizeof(float), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

int pt_variance(int samples, float *var_mean_host) {
    PTCHECK(moments_refusals("pt_variance"));
    if (!var_mean_host) return fail(PT_ERR_INVALID, "pt_variance: null");
    if (samples < 2) return fail(PT_ERR_INVALID, "pt_variance: samples must be >= 2 (a variance needs two)");
    if (!R().dnVar.p) PTCHECK(R().dnVar.alloc((size_t)R().P));
    hipLaunchKernelGGL(k_variance, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().image, R().moments.p, R().P, (float)samples,
                       (float)(samples - 1), R().dnVar.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(var_mean_host, R().dnVar.p, (size_t)R().P * sizeof(float), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

int pt_denoise_var(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, float *rgb_mean_host, float *var_host) {
    return denoise_var_to_host(samples, p, params_struct_bytes, kAtrousAuto, nullptr, rgb_mean_host, var_host, "pt_denoise_var");
}

int pt_denoise_var_rgba8(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, uint8_t *rgba_host) {
    if (!rgba_host) return fail(PT_ERR_INVALID, "pt_denoise_var_rgba8: null");
    PTCHECK(denoise_var_run(samples, p, params_struct_bytes, kAtrousAuto, false, nullptr, "pt_denoise_var_rgba8"));
    if (!R().dnRgba.p) PTCHECK(R().dnRgba.alloc((size_t)R().P));
    hipLaunchKernelGGL(k_to_rgba8, dim3((R().P + kBlock - 1) / kBlock), dim3(kBlock), 0, R().stream, R().dnOut.p, R().P, 1, R().dnRgba.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(rgba_host, R().dnRgba.p, (size_t)R().P * 4, hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

// ---- the noise statistics of 16 x 16 tiles, and rendering until they pass (pt_noise.h) -----------------------------------------------------
int pt_noise_stats(int samples, float threshold, float lum_floor, PtNoiseStats *out, size_t stats_struct_bytes, float *tile_rel_var_host) {
    PTCHECK(moments_refusals("pt_noise_stats"));
    if (!out || stats_struct_bytes != sizeof(PtNoiseStats))
        return fail(PT_ERR_INVALID, "pt_noise_stats: the caller's PtNoiseStats is %zu bytes, this library's %zu", out ? stats_struct_bytes : (size_t)0,
                    sizeof(PtNoiseStats));
    if (samples < 2) return fail(PT_ERR_INVALID, "pt_noise_stats: samples must be >= 2 (a variance needs two)");
    if (!noise_positive(threshold) || !noise_positive(lum_floor)) return fail(PT_ERR_INVALID, "pt_noise_stats: threshold and lum_floor must be finite and > 0");
    PTCHECK(noise_buffers());
    const int W = R().prm.W, H = R().prm.H;
    const size_t tiles = (size_t)((W + kNoiseTile - 1) / kNoiseTile) * (size_t)((H + kNoiseTile - 1) / kNoiseTile);
    if (tile_rel_var_host && !R().noiseMap.p) PTCHECK(R().noiseMap.alloc(tiles));
    const float thr2 = threshold * threshold;
    PTCHECK(noise_launch(R().image, R().moments.p, W, H, samples, lum_floor, thr2, R().noiseFrame.p, tile_rel_var_host ? R().noiseMap.p : nullptr,
                         R().noiseHost, R().stream));
    if (tile_rel_var_host) HIPCHECK(hipMemcpyAsync(tile_rel_var_host, R().noiseMap.p, tiles * sizeof(float), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    noise_fill(out, W, H, samples, thr2, R().noiseHost, 0.0f);
    return readback_fault();
}

int pt_iterate_until(int frame, int first_iter, const PtNoiseTarget *t, size_t target_struct_bytes, PtNoiseStats *out, int32_t *samples_done) {
    PTCHECK(moments_refusals("pt_iterate_until"));
    if (!t || target_struct_bytes != sizeof(PtNoiseTarget))
        return fail(PT_ERR_INVALID, "pt_iterate_until: the caller's PtNoiseTarget is %zu bytes, this library's %zu", t ? target_struct_bytes : (size_t)0,
                    sizeof(PtNoiseTarget));
    if (!out) return fail(PT_ERR_INVALID, "pt_iterate_until: null");
    if (R().flags & PT_FLAG_TRACE_AHEAD) return fail(PT_ERR_INVALID, "pt_iterate_until: not with PT_FLAG_TRACE_AHEAD (the loop enqueues its own batches)");
    if (!noise_positive(t->threshold) || !noise_positive(t->lum_floor))
        return fail(PT_ERR_INVALID, "pt_iterate_until: threshold and lum_floor must be finite and > 0");
    if (!(t->max_unconverged_fraction >= 0.0f && t->max_unconverged_fraction <= 1.0f))
        return fail(PT_ERR_INVALID, "pt_iterate_until: max_unconverged_fraction must be 0..1");
    if (t->min_samples < 2) return fail(PT_ERR_INVALID, "pt_iterate_until: min_samples must be >= 2 (a variance needs two)");
    if (t->check_every < 1) return fail(PT_ERR_INVALID, "pt_iterate_until: check_every must be >= 1");
    if (first_iter < 1) return fail(PT_ERR_INVALID, "pt_iterate_until: first_iter must be >= 1");
    if (t->max_samples < first_iter) return fail(PT_ERR_INVALID, "pt_iterate_until: max_samples lies before first_iter");
    if (t->max_samples < 2 || t->max_samples >= kIterEnd)
        return fail(PT_ERR_INVALID, "pt_iterate_until: max_samples must be 2..4194303 (a variance needs two; seed bits, pathtrace.cu:43)");
    if (t->lookahead != 0 && t->lookahead != 1) return fail(PT_ERR_INVALID, "pt_iterate_until: lookahead must be 0 or 1");
    PTCHECK(noise_buffers());
    const int W = R().prm.W, H = R().prm.H;
    const float thr2 = t->threshold * t->threshold, frac = t->max_unconverged_fraction;
    int s = first_iter - 1;          // the samples the accumulator holds behind everything enqueued
    int pending = -1, pendingAt = 0; // the page-locked copy of a check that is in flight, and the sample count it judges
    int statsAt = 0;                 // `out` holds the statistics of that many samples (0: of nothing yet)
    int checks = 0;
    bool converged = false;
    // wait for the check in flight -- its event alone: the stream may already hold the next round -- and judge it
    auto resolve = [&]() -> int {
        HIPCHECK(hipEventSynchronize(R().noiseEv[pending]));
        noise_fill(out, W, H, pendingAt, thr2, R().noiseHost + 2 * pending, frac);
        statsAt = pendingAt;
        pending = -1;
        converged = out->converged != 0;
        return PT_OK;
    };
    while (s < t->max_samples && !converged) {
        const int round = std::min(t->check_every, t->max_samples - s);
        for (int done = 0; done < round;) {
            const int b = std::min(R().maxBatch, round - done);
            PTCHECK(pt_iterate_batch(frame, s + 1 + done, b, nullptr));
            done += b;
        }
        s += round;
        if (pending >= 0) {          // lookahead: the round just enqueued counts whichever way the check before it went
            PTCHECK(resolve());
            if (converged) break;
        }
        if (s < t->min_samples) continue;
        pending = checks++ & 1;
        pendingAt = s;
        PTCHECK(noise_enqueue_check(pending, s, t->lum_floor, thr2));
        if (t->lookahead == 0 || s == t->max_samples) PTCHECK(resolve());
    }
    if (statsAt != s) {              // the final accumulator's statistics: a lookahead round came after the last check, or none was due
        const bool how = converged;
        pending = checks++ & 1;
        pendingAt = s;
        PTCHECK(noise_enqueue_check(pending, s, t->lum_floor, thr2));
        PTCHECK(resolve());
        converged = how;
    }
    out->converged = converged ? 1 : 0;
    if (samples_done) *samples_done = s;
    return check_device_fault();
}

int pt_gbuffer(int guide_iter, float *pos_t_host, float *nrm_host, int32_t *geom_host) {
    int rc = denoise_refusals("pt_gbuffer");
    if (rc) return rc;
    if (!pos_t_host || !nrm_host || !geom_host) return fail(PT_ERR_INVALID, "pt_gbuffer: null");
    rc = ensure_guides(guide_iter, nullptr);
    if (rc) return rc;
    const size_t P = (size_t)R().P;
    std::vector<float> tmp(P * 4);
    HIPCHECK(hipMemcpyAsync(pos_t_host, R().dnPosT.p, P * sizeof(float4), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipMemcpyAsync(tmp.data(), R().dnNrmId.p, P * sizeof(float4), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    for (size_t i = 0; i < P; ++i) {
        memcpy(nrm_host + 3 * i, tmp.data() + 4 * i, 3 * sizeof(float));
        memcpy(geom_host + i, tmp.data() + 4 * i + 3, sizeof(int32_t));
    }
    return readback_fault();
}

int pt_counters(PtCounters *out) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_counters before pt_init");
    if (!out) return fail(PT_ERR_INVALID, "pt_counters: null");
    int rc = sync_all();
    if (rc) return rc;
    rc = resolve_events(R().evBounce, R().msBounce, R().nBounce);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    std::unique_ptr<Ctrl> hp(new Ctrl);   // 2 MB: off the stack, and not shared by the host threads that drive other contexts
    Ctrl &h = *hp;
    uint32_t faultBits = 0;
    for (int i = 0; i < R().nslots; ++i) {
        HIPCHECK(hipMemcpy(&h, R().slot[i].ctrl.p, sizeof h, hipMemcpyDeviceToHost));
        for (int d = 0; d < kMaxDepthSlots; ++d) {
            int64_t early = 0;
            for (int sg = 0; sg < kTallyShards; ++sg) early += (int64_t)h.early[d][sg][0];
            out->live[d] += (int64_t)h.sum_live[d] + early;   // they did enter bounce d
            out->ended_early[d] += early;                      // ... without being moved through memory
        }
        for (int sg = 0; sg < kTallyShards; ++sg) {
            out->light_hits += (int64_t)h.light_hits[sg][0];
            out->misses += (int64_t)h.misses[sg][0];
        }
        faultBits |= h.error;
    }
    out->iterations = R().iterations;
    out->bounce_launches = R().nBounce;
    out->bounce_kernel_ms = R().msBounce;
    out->raygen_kernel_ms = 0.0;   // camera rays are generated inside the first bounce launch
    out->raygen_launches = 0;
    if (faultBits) return fail(PT_ERR_DEVICE, "%s", fault_message(faultBits).c_str());
    return PT_OK;
}

int pt_counters_reset(void) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_counters_reset before pt_init");
    int rc = sync_all();
    if (rc) return rc;
    rc = resolve_events(R().evBounce, R().msBounce, R().nBounce);
    if (rc) return rc;
    R().msBounce = 0;
    R().nBounce = 0;
    R().iterations = 0;
    for (int i = 0; i < R().nslots; ++i) {
        // the sticky fault word survives a counter reset
        uint32_t err = 0;
        HIPCHECK(hipMemcpy(&err, &R().slot[i].ctrl.p->error, sizeof err, hipMemcpyDeviceToHost));
        rc = reset_ctrl(R().slot[i].ctrl.p, nullptr);
        if (rc) return rc;
        R().slot[i].parity = 0;
        if (err) HIPCHECK(hipMemcpy(&R().slot[i].ctrl.p->error, &err, sizeof err, hipMemcpyHostToDevice));
    }
    return PT_OK;
}

// ---- stream compaction library -------------------------------------------------------------------------
int pt_scan_exclusive_i32(const int32_t *in_dev, int32_t *out_dev, int64_t n, void *stream) {
    if (n < 0 || (n > 0 && (!in_dev || !out_dev))) return fail(PT_ERR_INVALID, "pt_scan_exclusive_i32: bad argument");
    if (n == 0) return PT_OK;
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device");
    if (n > (1ll << 42)) return fail(PT_ERR_INVALID, "pt_scan_exclusive_i32: n too large");
    hipStream_t st = (hipStream_t)stream;
    register_exit_handler();
    std::lock_guard<std::mutex> lock(g_scanMutex);   // (look-up AND launches: see scan_ws)
    ScanWs *wp = nullptr;
    int rc = scan_ws(st, &wp);
    if (rc) return rc;
    long long per;
    int chunks;
    scan_chunks(n, &per, &chunks);
    // Two launches (12 bytes of HBM traffic per element).  PT_AMD_SCAN=1: the ONE-launch form (k_scan_chained: ticketed chunks, chained
    // prefix; 8 bytes per element when a chunk's second read comes out of the caches) -- measured SLOWER on MI355X, 0.214 against 0.172 ms at
    // 2^26 (0.81 against 0.66 at 2^28): the 2048 resident workgroups' chunks (128 KB each) do not survive in the 4 MB L2 of an XCD between
    // their two reads, so it moves the same 12 bytes and adds the ticket and the wait; kept selectable, not the default.
    const char *mode = getenv("PT_AMD_SCAN");
    if (!(mode && atoi(mode) == 1)) {
        // (chunks of four tiles or more take the kernels that load a tile ahead; the apply adds up the totals before its chunk itself)
        if (per >= 4) hipLaunchKernelGGL((k_scan_reduce<false, true>), dim3(chunks), dim3(kBlock), 0, st, in_dev, (long long)n, per, wp->partial.p);
        else hipLaunchKernelGGL((k_scan_reduce<false, false>), dim3(chunks), dim3(kBlock), 0, st, in_dev, (long long)n, per, wp->partial.p);
        if (per >= 4) hipLaunchKernelGGL((k_scan_apply<true>), dim3(chunks), dim3(kBlock), 0, st, in_dev, out_dev, (long long)n, per, wp->partial.p);
        else hipLaunchKernelGGL((k_scan_apply<false>), dim3(chunks), dim3(kBlock), 0, st, in_dev, out_dev, (long long)n, per, wp->partial.p);
    } else {
        if (++wp->gen == 0u) ++wp->gen;
        HIPCHECK(hipMemsetAsync(wp->chained.p, 0, sizeof(uint32_t), st));          // the ticket (the sums are tagged with the call's generation)
        hipLaunchKernelGGL(k_scan_chained, dim3(chunks), dim3(kBlock), 0, st, in_dev, out_dev, (long long)n, per, wp->chained.p, wp->gen);
    }
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

int pt_compact_nonzero_i32(const int32_t *in_dev, int32_t *out_dev, int64_t n, int64_t *count_dev, void *stream) {
    if (n < 0 || !count_dev || (n > 0 && (!in_dev || !out_dev))) return fail(PT_ERR_INVALID, "pt_compact_nonzero_i32: bad argument");
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device");
    if (n > 0xffffffffll) return fail(PT_ERR_INVALID, "pt_compact_nonzero_i32: n too large (positions are 32-bit)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHECK(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st));
        return PT_OK;
    }
    register_exit_handler();
    std::lock_guard<std::mutex> lock(g_scanMutex);   // (look-up AND launches: see scan_ws)
    ScanWs *wp = nullptr;
    int rc = scan_ws(st, &wp);
    if (rc) return rc;
    long long per;
    int chunks;
    scan_chunks(n, &per, &chunks);
    if (per >= 4) hipLaunchKernelGGL((k_scan_reduce<true, true>), dim3(chunks), dim3(kBlock), 0, st, in_dev, (long long)n, per, wp->partial.p);
    else hipLaunchKernelGGL((k_scan_reduce<true, false>), dim3(chunks), dim3(kBlock), 0, st, in_dev, (long long)n, per, wp->partial.p);
    if (per >= 4)
        hipLaunchKernelGGL((k_compact_apply<true>), dim3(chunks), dim3(kBlock), 0, st, in_dev, out_dev, (long long)n, per, wp->partial.p, reinterpret_cast<long long *>(count_dev));
    else
        hipLaunchKernelGGL((k_compact_apply<false>), dim3(chunks), dim3(kBlock), 0, st, in_dev, out_dev, (long long)n, per, wp->partial.p, reinterpret_cast<long long *>(count_dev));
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

#include "pt_group.h"

#ifdef PT_TEST_API
#include "pt_test_api.h"
#endif  // PT_TEST_API

}  // extern "C"
#pragma GCC visibility pop
