// Stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer over the comparison PT_FLAG_KEEP_RENDERER makes between a full
// pt_init call and what the live renderer was initialised with (csrc/pt_scene_plan.h: keep_renderer_mismatch): host code only, no device,
// nothing loaded into an interpreter.  tests/run_keep_renderer_sanitizer.sh compiles it with -fsanitize=address,undefined and runs it.
// The cases are those of tests/test_gpu_keep_renderer.py's second test, as plain arrays: the renderer's copies against an equal call whose
// arrays live at other addresses (no difference), then against calls that differ in one thing each -- a material's colour, a geom's
// translation, traceDepth, max_batch, pipeline_depth, lens_radius, a flag bit, the resolution, a texel, a UV, a triangle vertex, a face
// material, a bump scale, a texture added, the meshes cleared -- and the edge cases of the routine itself: empty scenes, NULL arrays with a
// count, arrays of other lengths, the registered data being the renderer's own objects -- all four parts, or three of them with the
// fourth replaced.  Exit status 0 and "sanitizer run finished" when every answer is the expected one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../include/pt_amd.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_compaction.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_trace.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_mesh_walk.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_mesh.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_camera_faces.h"

using namespace ptd;
using namespace ptk;

namespace {
std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define PTCHECK(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
bool env_flag(const char *name) { const char *e = getenv(name); return e && atoi(e); }
#include "../project3-cuda-path-tracer_amd/csrc/pt_host_scene.h"
#include "../project3-cuda-path-tracer_amd/csrc/pt_scene_plan.h"

// one side of the comparison, owning its arrays (exactly sized on the heap: a read past an end is the sanitizer's to find)
struct Side {
    std::vector<PtGeom> geoms;
    std::vector<PtMaterial> mats;
    int depth = 3;
    PtOptions o;
    int W = 48, H = 32;
    std::vector<ptm::HostMesh> meshes;
    std::vector<HostTexture> textures;
    std::vector<HostTexBinding> texBindings;
    std::vector<HostBumpBinding> bumpBindings;
    // (the registrations as a pt_set_* call leaves them: every part a fresh object)
    Registered reg() const {
        Registered r;
        r.meshes = std::make_shared<const std::vector<ptm::HostMesh>>(meshes);
        r.textures = std::make_shared<const std::vector<HostTexture>>(textures);
        r.texBindings = std::make_shared<const std::vector<HostTexBinding>>(texBindings);
        r.bumpBindings = std::make_shared<const std::vector<HostBumpBinding>>(bumpBindings);
        return r;
    }
    InitCall call() const { return InitCall{geoms.data(), (int)geoms.size(), mats.data(), (int)mats.size(), depth, &o, W, H, reg()}; }
};

Side base() {
    Side s;
    s.geoms.resize(8);
    s.mats.resize(5);
    for (size_t i = 0; i < s.geoms.size(); ++i) {
        memset(&s.geoms[i], 0, sizeof(PtGeom));
        s.geoms[i].type = i == 7 ? PT_MESH : (i % 2 ? PT_CUBE : PT_SPHERE);
        s.geoms[i].materialid = (int)(i % 5);
        s.geoms[i].translation = PtVec3{(float)i, 1.0f, -2.0f};
        for (int d = 0; d < 4; ++d) s.geoms[i].transform[5 * d] = s.geoms[i].inverseTransform[5 * d] = s.geoms[i].invTranspose[5 * d] = 1.0f;
    }
    for (size_t i = 0; i < s.mats.size(); ++i) {
        memset(&s.mats[i], 0, sizeof(PtMaterial));
        s.mats[i].color = PtVec3{0.1f * (float)i, 0.5f, 0.9f};
    }
    s.o = effective_options(nullptr);
    s.o.flags = PT_FLAG_MOMENTS | PT_FLAG_KEEP_RENDERER;
    s.o.max_batch = 4;
    s.o.pipeline_depth = 3;
    ptm::HostMesh m;
    m.geom = 7;
    m.tris.resize(9 * 12);
    for (size_t i = 0; i < m.tris.size(); ++i) m.tris[i] = 0.01f * (float)i;
    m.mats.assign(12, -1);
    s.meshes.push_back(m);
    for (int t = 0; t < 3; ++t) {
        HostTexture tx;
        tx.w = 4 << t; tx.h = 2 << t;
        tx.rgb.resize((size_t)tx.w * tx.h * 3);
        for (size_t i = 0; i < tx.rgb.size(); ++i) tx.rgb[i] = (float)((i * 7 + t) % 13) / 13.0f;
        s.textures.push_back(tx);
    }
    HostTexBinding tb;
    tb.geom = 7; tb.texture = 2; tb.ntris = 12;
    tb.uvs.resize(6 * 12);
    for (size_t i = 0; i < tb.uvs.size(); ++i) tb.uvs[i] = (float)(i % 6) / 6.0f;
    s.texBindings.push_back(tb);
    HostBumpBinding bb;
    bb.geom = 3; bb.texture = 0; bb.ntris = 0; bb.scale = 0.05f;
    s.bumpBindings.push_back(bb);
    bb.geom = 7; bb.texture = 1; bb.ntris = 12; bb.scale = 0.02f; bb.uvs = tb.uvs;
    s.bumpBindings.push_back(bb);
    return s;
}

int g_bad = 0, g_cases = 0;
void expect(const char *name, const Side &now, const Side &then, const char *want) {
    const char *got = keep_renderer_mismatch(now.call(), then.call());
    ++g_cases;
    const bool ok = want ? (got && !strcmp(got, want)) : !got;
    if (!ok) { fprintf(stderr, "%s: expected %s, got %s\n", name, want ? want : "(equal)", got ? got : "(equal)"); ++g_bad; }
}
}  // namespace

int main() {
    const Side then = base();
    {   // equal content at other addresses (every vector of `now` is a fresh allocation)
        const Side now = base();
        expect("equal", now, then, nullptr);
        expect("equal, the other way", then, now, nullptr);
        expect("itself", then, then, nullptr);
    }
    struct Case { const char *name; std::function<void(Side &)> change; const char *want; };
    const Case cases[] = {
        {"material colour", [](Side &s) { s.mats[1].color.x = 0.31f; }, "materials"},
        {"geom translation", [](Side &s) { s.geoms[4].translation.y += 0.25f; }, "geoms"},
        {"last byte of the geoms", [](Side &s) { s.geoms.back().invTranspose[15] = 2.0f; }, "geoms"},
        {"traceDepth", [](Side &s) { s.depth = 4; }, "traceDepth"},
        {"max_batch", [](Side &s) { s.o.max_batch = 2; }, "max_batch"},
        {"pipeline_depth", [](Side &s) { s.o.pipeline_depth = 2; }, "pipeline_depth"},
        {"lens_radius", [](Side &s) { s.o.lens_radius = 0.1f; }, "lens_radius"},
        {"focal_distance", [](Side &s) { s.o.focal_distance = 9.0f; }, "focal_distance"},
        {"flag bit", [](Side &s) { s.o.flags |= PT_FLAG_MIXTURE_WEIGHTED; }, "flags"},
        {"the flag itself", [](Side &s) { s.o.flags &= ~PT_FLAG_KEEP_RENDERER; }, "flags"},
        {"shard", [](Side &s) { s.o.shard_count = 2; }, "shard"},
        {"device", [](Side &s) { s.o.device = 0; }, "device"},
        {"stream", [](Side &s) { s.o.stream = (void *)&s; }, "stream"},
        {"accum_dev", [](Side &s) { s.o.accum_dev = (float *)&s; }, "accum_dev"},
        {"resolution", [](Side &s) { s.W = 37; s.H = 23; }, "resolution"},
        {"texel", [](Side &s) { s.textures[0].rgb[3] += 0.125f; }, "texels"},
        {"last texel", [](Side &s) { s.textures[2].rgb.back() += 0.125f; }, "texels"},
        {"texture size, same texel count", [](Side &s) { std::swap(s.textures[1].w, s.textures[1].h); }, "texture size"},
        {"uv", [](Side &s) { s.texBindings[0].uvs[62] += 0.0625f; }, "texture UVs"},
        {"binding's texture", [](Side &s) { s.texBindings[0].texture = 1; }, "texture binding"},
        {"triangle vertex", [](Side &s) { s.meshes[0].tris[17 * 4] += 0.03125f; }, "mesh triangles"},
        {"one triangle fewer", [](Side &s) { s.meshes[0].tris.resize(9 * 11); }, "mesh triangles"},
        {"face material", [](Side &s) { s.meshes[0].mats[5] = 1; }, "mesh face materials"},
        {"face materials dropped", [](Side &s) { s.meshes[0].mats.clear(); }, "mesh face materials"},
        {"normals added", [](Side &s) { s.meshes[0].normals.assign(9 * 12, 0.5f); }, "mesh normals"},
        {"mesh of another geom", [](Side &s) { s.meshes[0].geom = 6; }, "mesh geom"},
        {"bump scale", [](Side &s) { s.bumpBindings[0].scale = 0.08f; }, "bump scale"},
        {"bump uv", [](Side &s) { s.bumpBindings[1].uvs[0] = 0.75f; }, "bump UVs"},
        {"bump binding dropped", [](Side &s) { s.bumpBindings.pop_back(); }, "bump binding count"},
        {"texture added", [](Side &s) { HostTexture t; t.w = t.h = 2; t.rgb.assign(12, 0.5f); s.textures.push_back(t); }, "texture count"},
        {"textures cleared", [](Side &s) { s.textures.clear(); }, "texture count"},
        {"bindings cleared", [](Side &s) { s.texBindings.clear(); }, "texture binding count"},
        {"meshes cleared", [](Side &s) { s.meshes.clear(); }, "mesh count"},
        {"a geom fewer", [](Side &s) { s.geoms.pop_back(); }, "geom count"},
        {"a material more", [](Side &s) { s.mats.push_back(s.mats[0]); }, "material count"},
        {"minus zero for zero", [](Side &s) { s.geoms[0].rotation.x = -0.0f; }, "geoms"},
    };
    for (const Case &c : cases) {
        Side now = base();
        c.change(now);
        expect(c.name, now, then, c.want);
        expect(c.name, then, now, c.want);
    }
    {   // the routine's own edge cases: empty scenes, NULL arrays, missing options, registered data shared between the two sides
        Side a = base(), b = base();
        a.geoms.clear(); a.mats.clear(); b.geoms.clear(); b.mats.clear();
        expect("two empty scenes", a, b, nullptr);
        const Side full = base();
        InitCall nul = full.call();
        nul.geoms = nullptr;
        ++g_cases;
        if (!keep_renderer_mismatch(nul, then.call())) { fprintf(stderr, "NULL geoms with a count matched\n"); ++g_bad; }
        nul = full.call();
        nul.mats = nullptr;
        ++g_cases;
        if (!keep_renderer_mismatch(nul, then.call())) { fprintf(stderr, "NULL materials with a count matched\n"); ++g_bad; }
        nul = full.call();
        nul.o = nullptr;
        ++g_cases;
        if (!keep_renderer_mismatch(nul, then.call())) { fprintf(stderr, "missing options matched\n"); ++g_bad; }
        nul = full.call();
        nul.ngeoms = -1;
        InitCall neg = then.call();
        neg.ngeoms = -1;
        ++g_cases;
        if (!keep_renderer_mismatch(nul, neg)) { fprintf(stderr, "a negative count matched\n"); ++g_bad; }
        InitCall shared = full.call();
        shared.reg = then.call().reg;       // (no pt_set_* call since the renderer's pt_init: one set of objects)
        ++g_cases;
        if (keep_renderer_mismatch(shared, then.call())) { fprintf(stderr, "shared registrations differ\n"); ++g_bad; }
    }
    {   // two sets of registrations that share three parts -- no pt_set_* call has replaced those -- and differ in the fourth, each part in
        // turn: the mismatch is that part's first comparison; and a fourth part that is another object with the same bytes matches
        const Side full = base();
        Side fewer = base();
        fewer.meshes.clear(); fewer.textures.pop_back(); fewer.texBindings.clear(); fewer.bumpBindings.pop_back();
        const Registered mine = full.reg(), equal = full.reg(), other = fewer.reg();
        struct Part { const char *name, *want; std::function<void(Registered &, const Registered &)> take; };
        const Part parts[] = {
            {"meshes", "mesh count", [](Registered &r, const Registered &from) { r.meshes = from.meshes; }},
            {"textures", "texture count", [](Registered &r, const Registered &from) { r.textures = from.textures; }},
            {"texture bindings", "texture binding count", [](Registered &r, const Registered &from) { r.texBindings = from.texBindings; }},
            {"bump bindings", "bump binding count", [](Registered &r, const Registered &from) { r.bumpBindings = from.bumpBindings; }},
        };
        for (const Part &part : parts) {
            InitCall a = full.call(), b = full.call();
            a.reg = b.reg = mine;
            part.take(b.reg, other);
            for (int way = 0; way < 2; ++way) {
                const char *got = way ? keep_renderer_mismatch(b, a) : keep_renderer_mismatch(a, b);
                ++g_cases;
                if (!got || strcmp(got, part.want)) { fprintf(stderr, "three parts shared, other %s: expected %s, got %s\n", part.name, part.want, got ? got : "(equal)"); ++g_bad; }
            }
            part.take(b.reg, equal);
            ++g_cases;
            if (const char *got = keep_renderer_mismatch(a, b)) { fprintf(stderr, "three parts shared, equal %s in another object: got %s\n", part.name, got); ++g_bad; }
        }
        InitCall a = full.call(), b = full.call();
        a.reg = mine; b.reg = equal;
        ++g_cases;
        if (keep_renderer_mismatch(a, b)) { fprintf(stderr, "four distinct parts with equal bytes differ\n"); ++g_bad; }
    }
    printf("%d comparisons, %d with an unexpected answer\n", g_cases, g_bad);
    if (g_bad) return 1;
    printf("sanitizer run finished\n");
    return 0;
}
