// pt_scene_plan.h -- the host half of pt_init: plan_scene() checks a scene and derives everything the renderer needs before it needs a
// device -- KParams, every table in its final state, the renderer's flags and sizes (ScenePlan) -- from its arguments alone.  No HIP runtime
// call, no renderer state: it runs without a GPU (pt_test_scene_plan, tests/test_scene_plan_cpu.py), and a scene it refuses has touched
// nothing.  pt_init (pt_api.hip) is the device half: it allocates, uploads each table once and sizes the launches.
// Included inside the anonymous namespace of pt_api.hip behind pt_host_scene.h, whose building blocks the steps below put together; the
// including file provides fail(), env_flag() and PTCHECK.
#pragma once

constexpr int kMaxSlots = 4;
constexpr int kTexSizeMax = 16384;     // largest side of a texture (pt_set_textures)
constexpr long long kTexTexelsMax = 1ll << 28;   // the textures of a scene hold fewer texels

// what pt_set_textures and pt_set_bump_maps registered, as the next pt_init reads it (texture: an index into the textures)
struct HostTexture { int w = 0, h = 0; std::vector<float> rgb; };              // rgb: w * h * 3, or empty where w or h is out of range
struct HostTexBinding { int geom = 0, texture = 0, ntris = 0; std::vector<float> uvs; };
struct HostBumpBinding { int geom = 0, texture = 0, ntris = 0; float scale = 0.0f; std::vector<float> uvs; };

// What the pt_set_* calls registered: meshes (pt_set_meshes), textures and their bindings (pt_set_textures), height maps (pt_set_bump_maps).
// A part is immutable once registered and shared by reference count: a pt_set_* call puts a new vector in the place of its part, and
// whoever copied the old one -- the live renderer, for its camera moves -- still holds it.  Never null: an empty vector stands for "none".
struct Registered {
    std::shared_ptr<const std::vector<ptm::HostMesh>> meshes = std::make_shared<const std::vector<ptm::HostMesh>>();
    std::shared_ptr<const std::vector<HostTexture>> textures = std::make_shared<const std::vector<HostTexture>>();
    std::shared_ptr<const std::vector<HostTexBinding>> texBindings = std::make_shared<const std::vector<HostTexBinding>>();
    std::shared_ptr<const std::vector<HostBumpBinding>> bumpBindings = std::make_shared<const std::vector<HostBumpBinding>>();
};

// The arguments of pt_init with the options made effective (pt_init's defaults where the caller gave none), and what the calls before it
// registered (the caller keeps its Registered while the SceneIn is read).
struct SceneIn {
    const PtCamera *cam;
    const PtGeom *geoms;
    int ngeoms;
    const PtMaterial *mats;
    int nmats, traceDepth;
    PtOptions o;
    const std::vector<ptm::HostMesh> &meshes;
    const std::vector<HostTexture> &textures;
    const std::vector<HostTexBinding> &texBindings;
    const std::vector<HostBumpBinding> &bumpBindings;
    SceneIn(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions &o, const Registered &reg)
        : cam(cam), geoms(geoms), ngeoms(ngeoms), mats(mats), nmats(nmats), traceDepth(traceDepth), o(o), meshes(*reg.meshes), textures(*reg.textures),
          texBindings(*reg.texBindings), bumpBindings(*reg.bumpBindings) {}
    // who evaluates the work list's face certificates between build_camera_list's two passes: nobody named -- the host (pt_init, the
    // host-only entry points); the camera move (pt_api.hip) names the device (k_camera_faces).  PT_OK, or what fail() returned.
    std::function<int(CameraGroups &, const CameraResolve &)> faces = nullptr;
    const ptm::HostMesh *mesh_of(int geom) const {
        for (const ptm::HostMesh &m : meshes)
            if (m.geom == geom) return &m;
        return nullptr;
    }
    bool direct() const { return (o.flags & PT_FLAG_DIRECT_LIGHTING) != 0; }
};

// pt_init's options where the caller gave none
PtOptions effective_options(const PtOptions *opts) {
    PtOptions o;
    memset(&o, 0, sizeof o);
    o.shard_count = 1;
    o.device = -1;
    if (opts) o = *opts;
    return o;
}

// PT_FLAG_KEEP_RENDERER: is a full pt_init call the one the live renderer was initialised with, the camera's pose aside?  `now`: the call's
// arguments (options made effective) and what is registered at this moment; `then`: the renderer's copies.  NULL where everything the flag's
// definition lists (include/pt_amd.h) is equal, else the name of the first comparison that failed (pt_test_keep_mismatch).  Arrays are
// compared byte for byte -- texels too: no hash --, so a -0.0 for a 0.0 is a difference: the full call, which is always right.
struct InitCall {
    const PtGeom *geoms;
    int ngeoms;
    const PtMaterial *mats;
    int nmats, traceDepth;
    const PtOptions *o;
    int W, H;
    Registered reg;      // (a part the two sides share -- one object -- is not compared byte for byte)
};
template <typename T>
inline bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}
// what two sets of registrations differ in -- counts, sizes and bindings, the triangle, normal, face-material and UV arrays, the texels, all
// byte for byte --, or NULL (PT_FLAG_KEEP_RENDERER; PT_FLAG_OBJECT_HISTORY's scene comparison)
inline const char *registered_mismatch(const Registered &p, const Registered &q) {
    if (p.meshes != q.meshes) {
        if (p.meshes->size() != q.meshes->size()) return "mesh count";
        for (size_t i = 0; i < p.meshes->size(); ++i) {
            const ptm::HostMesh &m = (*p.meshes)[i], &n = (*q.meshes)[i];
            if (m.geom != n.geom) return "mesh geom";
            if (!same_bytes(m.tris, n.tris)) return "mesh triangles";
            if (!same_bytes(m.normals, n.normals)) return "mesh normals";
            if (!same_bytes(m.mats, n.mats)) return "mesh face materials";
        }
    }
    if (p.textures != q.textures) {
        if (p.textures->size() != q.textures->size()) return "texture count";
        for (size_t i = 0; i < p.textures->size(); ++i) {
            const HostTexture &s = (*p.textures)[i], &t = (*q.textures)[i];
            if (s.w != t.w || s.h != t.h) return "texture size";
            if (!same_bytes(s.rgb, t.rgb)) return "texels";
        }
    }
    if (p.texBindings != q.texBindings) {
        if (p.texBindings->size() != q.texBindings->size()) return "texture binding count";
        for (size_t i = 0; i < p.texBindings->size(); ++i) {
            const HostTexBinding &s = (*p.texBindings)[i], &t = (*q.texBindings)[i];
            if (s.geom != t.geom || s.texture != t.texture || s.ntris != t.ntris) return "texture binding";
            if (!same_bytes(s.uvs, t.uvs)) return "texture UVs";
        }
    }
    if (p.bumpBindings != q.bumpBindings) {
        if (p.bumpBindings->size() != q.bumpBindings->size()) return "bump binding count";
        for (size_t i = 0; i < p.bumpBindings->size(); ++i) {
            const HostBumpBinding &s = (*p.bumpBindings)[i], &t = (*q.bumpBindings)[i];
            if (s.geom != t.geom || s.texture != t.texture || s.ntris != t.ntris) return "bump binding";
            if (memcmp(&s.scale, &t.scale, sizeof(float))) return "bump scale";
            if (!same_bytes(s.uvs, t.uvs)) return "bump UVs";
        }
    }
    return nullptr;
}
inline const char *keep_renderer_mismatch(const InitCall &now, const InitCall &then) {
    if (!now.o || !then.o) return "options";
    if (now.W != then.W || now.H != then.H) return "resolution";
    if (now.ngeoms != then.ngeoms || now.ngeoms < 0 || (now.ngeoms > 0 && (!now.geoms || !then.geoms))) return "geom count";
    if (now.nmats != then.nmats || now.nmats < 0 || (now.nmats > 0 && (!now.mats || !then.mats))) return "material count";
    if (now.ngeoms > 0 && memcmp(now.geoms, then.geoms, (size_t)now.ngeoms * sizeof(PtGeom))) return "geoms";
    if (now.nmats > 0 && memcmp(now.mats, then.mats, (size_t)now.nmats * sizeof(PtMaterial))) return "materials";
    if (now.traceDepth != then.traceDepth) return "traceDepth";
    const PtOptions &a = *now.o, &b = *then.o;
    if (a.shard_rank != b.shard_rank || a.shard_count != b.shard_count) return "shard";
    if (a.device != b.device) return "device";
    if (a.flags != b.flags) return "flags";
    if (a.pipeline_depth != b.pipeline_depth) return "pipeline_depth";
    if (a.max_batch != b.max_batch) return "max_batch";
    if (a.stream != b.stream) return "stream";
    if (a.accum_dev != b.accum_dev) return "accum_dev";
    if (memcmp(&a.lens_radius, &b.lens_radius, sizeof(float))) return "lens_radius";
    if (memcmp(&a.focal_distance, &b.focal_distance, sizeof(float))) return "focal_distance";
    return registered_mismatch(now.reg, then.reg);
}

// bits of one code of a path's material history (ptk::PathPool): 2 * material + (specular ? 1 : 0) < 2 nmats -- max(1, ceil(log2(2 nmats)))
inline int history_code_bits(int nmats) {
    int b = 1;
    while ((1ll << b) < 2ll * nmats) ++b;
    return b;
}

// dynamic LDS k_gbuffer needs for a scene: the lanes' mesh traversal stacks (a launch holds at most 64 KB)
inline size_t guideStackBytes(bool mesh, int meshStackNeed) { return mesh ? (size_t)std::max(meshStackNeed, 1) * kBlock * sizeof(uint32_t) : 0; }

// What the renderer keeps of a plan (State derives from it): the launches read these on every call.
struct PlanScalars {
    PtCamera cam;
    KParams prm;            // complete except tilesPerRow, which depends on the grid (pt_init)
    int P = 0;              // W*H
    int nLocal = 0;
    int flags = 0;          // PtOptions::flags, PT_FLAG_TRACE_AHEAD stripped where max_batch is 1
    int nslots = 0;
    int maxBatch = 1;       // iterations that may share one wavefront (pt_iterate_batch)
    // which form of k_bounce a launch takes (bounce_form)
    bool grouped = false;   // hundreds of swept primitives: the later bounces take the k_bounce<..., GROUPS> instantiations
    bool tex = false;       // a texture is bound to at least one primitive (or a height map: BUMP forms are TEX forms)
    bool bump = false;      // a height map is bound to at least one primitive
    bool mesh = false;      // the scene holds triangle meshes: the k_bounce<., false, ., true> variants
    bool many = false;      // more than kBinMax small primitives (spheres, cubes that are neither walls nor binned): the k_bounce<., true> variants
    bool sweptCubes = false;  // ... some of them cubes (TileArgs::hot: kHotSweptCubes)
    bool dof = false;       // thin-lens camera: the k_bounce<true, ., true> variants for the camera-ray bounce
    bool plain = false;     // no refractive material, no specular exponent on a reflective one, no direct lighting: k_bounce<..., PLAIN>
    int meshStackNeed = 0;  // the stack levels a brute-force walk of the meshes needs per lane (k_gbuffer)
    // the meshes' walks (k_mesh_walk): the meshes alone per queue class / in all; walkMeshLds: how many WalkMesh rows a workgroup stages in LDS (all, or none)
    int walkMeshLds = 0;
    int walkClassOff[kClsMax + 1] = {0}, walkAll0 = 0, walkAll1 = 0;
    size_t ldsWalk = 0;
    size_t ldsBytes = 0, ldsBytesNext = 0;   // dynamic LDS of the camera-ray launch / of the later ones
    int numTilesMax = 0;    // upper bound of tiles in one bounce queue (incl. one partial tile per segment)
    int poolChunks = 0;     // chunks per path pool (incl. the trash chunk 0); a pool holds poolChunks * kChunk paths per array
    size_t poolCap = 0;     // ... that many paths
    size_t meshHitWords = 0;   // scenes with meshes: the walks' result words per slot (BounceArgs::meshHit), else 0
};

struct ScenePlan : PlanScalars {
    // the tables, each as it is uploaded
    std::vector<GeomDev> hg;
    std::vector<MaterialDev> hm;
    std::vector<unsigned char> geomHit;     // GeomHitDev[ngeoms], or a sphere-heavy scene's LDS image (plan_hit_records)
    std::vector<float> rowsGlobal;          // sphere-heavy scenes whose matrix rows stay out of LDS (BounceArgs::rows)
    std::vector<WallBox> hw;
    std::vector<SphereCull> sc, groups;
    std::vector<int> classIdx;
    CameraCull cc;                          // rowOff, rowIdx: the camera-ray bounce's per-row lists
    CameraList cl;                          // the packed work list, or empty
    std::vector<int> walkIdx, walkRowOff;
    std::vector<WalkMesh> walkMeshRows;
    std::vector<ptd::MeshUnit> meshRecs;    // (uploaded with 4 records of slack: a walk may read the record behind the last one)
    std::vector<ptd::TexGeom> texGeom;
    std::vector<int4> texDesc;
    std::vector<float4> texels, texUV;
    std::vector<ptd::BumpGeom> bumpGeom;
    std::vector<float4> bumpUV, bumpTan;
    // what one step leaves for the next
    int rows = 0;                           // image rows of this shard
    std::vector<std::array<float, 6>> meshBox;
    std::vector<const float *> boxes;       // per primitive: a mesh's object-space bounds (into meshBox), else nullptr
    std::vector<uint32_t> triBase;          // textured meshes: the unit of the first triangle record (ptm::appendMesh)
    int binGroup[kBinMax] = {0, 0, 0, 0};   // mesh scenes: the candidate bit of each binned primitive
    std::vector<char> swept;                // per primitive: swept per lane from the packed table `sc`
    int nswept = 0;
};

// A bumped mesh triangle's object-space tangents (ptd "bump mapping", mesh), fp32 in the order written there (this file is compiled
// with -ffp-contract=off for the host too): tri = its corners p0 p1 p2 (9 floats), uv = u0 v0 u1 v1 u2 v2 -> {Tu, det != 0}, {Tv, 0}
void meshTangents(const float *tri, const float *uv, float4 &tu, float4 &tv) {
    const float e1[3] = {tri[3] - tri[0], tri[4] - tri[1], tri[5] - tri[2]};
    const float e2[3] = {tri[6] - tri[0], tri[7] - tri[1], tri[8] - tri[2]};
    const float du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1], du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1];
    const float det = du1 * dv2 - du2 * dv1;
    float a[3], b[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = (e1[k] * dv2 - e2[k] * dv1) / det;
        b[k] = (e2[k] * du1 - e1[k] * du2) / det;
    }
    tu = make_float4(a[0], a[1], a[2], det != 0.0f ? 1.0f : 0.0f);
    tv = make_float4(b[0], b[1], b[2], 0.0f);
}

// a mesh binding's corner UVs (six floats per triangle) as the kernels read them: two float4 per triangle, {u0, v0, u1, v1}, {u2, v2, 0, 0}
void pack_uvs(const std::vector<float> &uvs, int ntris, std::vector<float4> &out) {
    for (int f = 0; f < ntris; ++f) {
        const float *c = uvs.data() + 6 * (size_t)f;
        out.push_back(make_float4(c[0], c[1], c[2], c[3]));
        out.push_back(make_float4(c[4], c[5], 0.0f, 0.0f));
    }
}

// magic_divisor for d, checked on the edges of every quotient range: n / d == (n * m) >> sh for the n < 2^30 the kernels divide
int checked_magic(uint32_t d, uint32_t &m, uint32_t &sh) {
    magic_divisor(d, m, sh);
    for (uint64_t q = 0; q * d < (1ull << 30); q = q < 64 ? q + 1 : q * 2 + 1)
        for (uint64_t n : {q * d, q * d + d - 1, (uint64_t)((1ull << 30) - 1) - q})
            if (n < (1ull << 30) && (uint32_t)((n * m) >> sh) != (uint32_t)(n / d))
                return fail(PT_ERR_INVALID, "pt_init: magic division self-check failed for d=%u n=%llu", d, (unsigned long long)n);
    return PT_OK;
}

// The camera-ray tiles' index space: nLocalPad entries in rows of Wp (a multiple of the tile size), and the divisors the kernels divide by the two with
int set_tile_space(KParams &k, int Wp, int nLocalPad) {
    k.Wp = Wp;
    k.nLocalPad = nLocalPad;
    PTCHECK(checked_magic((uint32_t)k.Wp, k.magicWp, k.shiftWp));
    return checked_magic((uint32_t)std::max(k.nLocalPad, 1), k.magicN, k.shiftN);
}

// does primitive i emit: its own material, or -- a mesh -- any of its faces' own materials
bool geom_emits(const SceneIn &in, int i) {
    bool emits = in.mats[in.geoms[i].materialid].emittance > 0.0f;
    if (in.geoms[i].type == PT_MESH)
        if (const ptm::HostMesh *m = in.mesh_of(i))
            for (int fm : m->mats) emits = emits || (fm >= 0 && fm < in.nmats && in.mats[fm].emittance > 0.0f);
    return emits;
}

// What every workgroup stages in LDS ahead of the scene's tables: the materials and the tile's bookkeeping words (ncls queue classes)
size_t lds_head(int nmats, int ncls) { return sizeof(MaterialDev) * nmats + (size_t)miscWords(ncls) * sizeof(uint32_t); }
// ... and the tables of a sphere-heavy scene behind them, in the kernel's own layout (k_bounce: S_GEOMHIT_SMALL .. behind S_SPH): the compact
// hit records, the cubes' face frames, the primitives' matrix rows (rowFloats of them: all, or none) and the sweep's entry -> primitive map
struct ManyLds {
    size_t hit, frames, rows, map;
    size_t tables() const { return hit + frames + rows; }
};
ManyLds many_lds(int ngeoms, int nCubes, int rowFloats, int nSphCull) {
    return ManyLds{manyHitBytes(ngeoms), (size_t)nCubes * 54 * sizeof(float) + manyFramePad(nCubes), (size_t)rowFloats * sizeof(float),
                   ((size_t)nSphCull + 7) / 8 * 8 * sizeof(uint16_t)};
}

// One binding of pt_set_textures (scale == nullptr) or pt_set_bump_maps against the scene; bound: which primitives a binding of the kind names already
int check_binding(const SceneIn &in, const float *scale, size_t index, int geom, int texture, int ntris, const std::vector<float> &uvs, std::vector<char> &bound) {
    const char *kind = scale ? "bump" : "texture", *meshKind = scale ? "bumped" : "textured", *bumped = scale ? "bumped " : "";
    if (geom < 0 || geom >= in.ngeoms) return fail(PT_ERR_INVALID, "pt_init: %s binding %zu names geom %d of %d", kind, index, geom, in.ngeoms);
    if (texture < 0 || texture >= (int)in.textures.size())
        return fail(PT_ERR_INVALID, "pt_init: %s binding %zu names texture %d of %zu", kind, index, texture, in.textures.size());
    if (bound[geom]++) return fail(PT_ERR_INVALID, "pt_init: geom %d has two %s bindings", geom, kind);
    if (scale && !std::isfinite(*scale)) return fail(PT_ERR_INVALID, "pt_init: bump binding %zu has a non-finite scale", index);
    if (in.geoms[geom].type == PT_MESH) {
        if (uvs.empty()) return fail(PT_ERR_INVALID, "pt_init: %s mesh geom %d has no UVs", meshKind, geom);
        const size_t have = in.mesh_of(geom)->tris.size();
        if ((size_t)ntris * 9 != have) return fail(PT_ERR_INVALID, "pt_init: UVs of %d triangles for %smesh geom %d of %zu", ntris, bumped, geom, have / 9);
    } else if (!uvs.empty() || ntris != 0) {
        return fail(PT_ERR_INVALID, "pt_init: UVs given for %sgeom %d, which is not a mesh", bumped, geom);
    }
    return PT_OK;
}

// ---- the steps of plan_scene, in its order ---------------------------------------------------------------------------------------------

// the arguments, the registered meshes, textures and bindings against the scene, the options
int check_scene(const SceneIn &in) {
    const PtCamera *cam = in.cam;
    const PtGeom *geoms = in.geoms;
    const PtOptions &o = in.o;
    const int ngeoms = in.ngeoms, nmats = in.nmats;
    if (!cam || ngeoms < 0 || nmats < 0 || (ngeoms && !geoms) || (nmats && !in.mats))
        return fail(PT_ERR_INVALID, "pt_init: null argument");
    if (cam->resolution[0] <= 0 || cam->resolution[1] <= 0) return fail(PT_ERR_INVALID, "pt_init: bad resolution");
    const bool direct = in.direct();
    if (in.traceDepth < 1 || in.traceDepth + (direct ? 1 : 0) > PT_MAX_DEPTH)
        return fail(PT_ERR_INVALID, "pt_init: traceDepth must be 1..%d", PT_MAX_DEPTH - (direct ? 1 : 0));
    if (!(o.lens_radius >= 0.0f) || (o.lens_radius > 0.0f && !(o.focal_distance > 0.0f)))
        return fail(PT_ERR_INVALID, "pt_init: lens_radius must be >= 0 and focal_distance > 0 with a lens");
    if ((long long)cam->resolution[0] * cam->resolution[1] > (1ll << 30)) return fail(PT_ERR_INVALID, "pt_init: frame too large");
    for (int i = 0; i < ngeoms; ++i) {
        if (geoms[i].type != PT_SPHERE && geoms[i].type != PT_CUBE && geoms[i].type != PT_MESH) return fail(PT_ERR_INVALID, "pt_init: geom %d has unknown type", i);
        if (geoms[i].type == PT_MESH && !in.mesh_of(i)) return fail(PT_ERR_INVALID, "pt_init: geom %d is a mesh without triangles (pt_set_meshes)", i);
        if (geoms[i].materialid < 0 || geoms[i].materialid >= nmats) return fail(PT_ERR_INVALID, "pt_init: geom %d references material %d", i, geoms[i].materialid);
    }
    for (const ptm::HostMesh &m : in.meshes)
        if (m.geom < 0 || m.geom >= ngeoms || geoms[m.geom].type != PT_MESH)
            return fail(PT_ERR_INVALID, "pt_init: triangles registered for geom %d, which is not a mesh of this scene (pt_set_meshes)", m.geom);
    long long texels = 0;
    for (size_t i = 0; i < in.textures.size(); ++i) {
        const HostTexture &t = in.textures[i];
        if (t.w < 1 || t.w > kTexSizeMax || t.h < 1 || t.h > kTexSizeMax)
            return fail(PT_ERR_INVALID, "pt_init: texture %zu is %d x %d (each side 1..%d)", i, t.w, t.h, kTexSizeMax);
        texels += (long long)t.w * t.h;
        if (texels >= kTexTexelsMax) return fail(PT_ERR_INVALID, "pt_init: the textures hold 2^28 texels or more");
        for (float c : t.rgb)
            if (!std::isfinite(c)) return fail(PT_ERR_INVALID, "pt_init: texture %zu holds a non-finite texel", i);
    }
    std::vector<char> bound(ngeoms, 0), bumped(ngeoms, 0);
    for (size_t i = 0; i < in.texBindings.size(); ++i) {
        const HostTexBinding &b = in.texBindings[i];
        PTCHECK(check_binding(in, nullptr, i, b.geom, b.texture, b.ntris, b.uvs, bound));
    }
    for (size_t i = 0; i < in.bumpBindings.size(); ++i) {
        const HostBumpBinding &b = in.bumpBindings[i];
        PTCHECK(check_binding(in, &b.scale, i, b.geom, b.texture, b.ntris, b.uvs, bumped));
    }
    if (o.shard_count < 1 || o.shard_rank < 0 || o.shard_rank >= o.shard_count) return fail(PT_ERR_INVALID, "pt_init: bad shard %d/%d", o.shard_rank, o.shard_count);
    if ((o.flags & PT_FLAG_MOMENTS) && (o.shard_count > 1 || (o.flags & PT_FLAG_ACCUM_SHARD_ROWS)))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_MOMENTS needs the whole frame: no row shard, no PT_FLAG_ACCUM_SHARD_ROWS");
    if (o.flags & PT_FLAG_TEMPORAL) {
        if (!(o.flags & PT_FLAG_MOMENTS)) return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_TEMPORAL needs PT_FLAG_MOMENTS (history carries the second moment)");
        if (o.flags & PT_FLAG_TRACE_AHEAD) return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_TEMPORAL is not for PT_FLAG_TRACE_AHEAD renderers");
        if (o.lens_radius > 0.0f) return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_TEMPORAL needs the pinhole camera (a thin lens has no single projection)");
    }
    if ((o.flags & PT_FLAG_DISPLAY_FILTER) && !(o.flags & PT_FLAG_MOMENTS))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DISPLAY_FILTER needs PT_FLAG_MOMENTS (the filter is guided by the variance)");
    if ((o.flags & PT_FLAG_SPATIAL_VARIANCE) && !(o.flags & PT_FLAG_MOMENTS))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_SPATIAL_VARIANCE needs PT_FLAG_MOMENTS (the estimate is made of the second moments)");
    if (o.flags & PT_FLAG_DEMODULATE) {
        if (!(o.flags & PT_FLAG_MOMENTS)) return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMODULATE needs PT_FLAG_MOMENTS (the filter it feeds is guided by the variance)");
        if ((o.flags & PT_FLAG_TEMPORAL) && !(o.flags & PT_FLAG_DEMOD_HISTORY))
            return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMODULATE is not for PT_FLAG_TEMPORAL renderers (history carries no albedo)");
        if (o.flags & PT_FLAG_TRACE_AHEAD)
            return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMODULATE is not for PT_FLAG_TRACE_AHEAD renderers (the albedo follows the committed iterations)");
    }
    if ((o.flags & PT_FLAG_DEMOD_HISTORY) && (~o.flags & (PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL | PT_FLAG_DEMODULATE)))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMOD_HISTORY needs PT_FLAG_MOMENTS, PT_FLAG_TEMPORAL and PT_FLAG_DEMODULATE (it joins the two)");
    if ((o.flags & PT_FLAG_OBJECT_HISTORY) && (~o.flags & (PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL)))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_OBJECT_HISTORY needs PT_FLAG_MOMENTS and PT_FLAG_TEMPORAL (it is the history that follows the objects)");
    if ((o.flags & PT_FLAG_MOTION) && (o.flags & (PT_FLAG_TEMPORAL | PT_FLAG_OBJECT_HISTORY | PT_FLAG_DISPLAY_FILTER | PT_FLAG_DEMODULATE |
                                                  PT_FLAG_SPATIAL_VARIANCE | PT_FLAG_KEEP_RENDERER)))
        return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_MOTION is not for PT_FLAG_TEMPORAL, PT_FLAG_OBJECT_HISTORY, PT_FLAG_DISPLAY_FILTER, PT_FLAG_DEMODULATE, "
                    "PT_FLAG_SPATIAL_VARIANCE or PT_FLAG_KEEP_RENDERER renderers (a first-hit guide, and a renderer kept across calls, have one pose)");
    if (o.pipeline_depth < 0 || o.pipeline_depth > kMaxSlots) return fail(PT_ERR_INVALID, "pt_init: pipeline_depth must be 0..%d", kMaxSlots);
    if (o.max_batch < 0 || o.max_batch > PT_MAX_BATCH) return fail(PT_ERR_INVALID, "pt_init: max_batch must be 0..%d", PT_MAX_BATCH);
    return PT_OK;
}

// the frame and this shard's rows of it; the camera, the lens, the depths; what the materials alone decide
int plan_frame(const SceneIn &in, ScenePlan &p) {
    const PtOptions &o = in.o;
    const int Wd = in.cam->resolution[0], H = in.cam->resolution[1];
    p.flags = o.flags;
    p.cam = *in.cam;
    p.P = Wd * H;
    p.rows = H > o.shard_rank ? (H - o.shard_rank + o.shard_count - 1) / o.shard_count : 0;
    p.nLocal = p.rows * Wd;

    KParams &k = p.prm;
    memset(&k, 0, sizeof k);
    camera_params(*in.cam, k);
    k.shardRank = o.shard_rank; k.shardCount = o.shard_count;
    k.nLocal = p.nLocal;
    magic_divisor((uint32_t)o.shard_count, k.magicS, k.shiftS);
    k.contribLocal = (o.shard_count > 1 && (long long)Wd * H < (1ll << 27)) ? 1 : 0;   // (the multiply-shift divisions hold below 2^27)
    // camera-ray tiles lie on rows padded to a multiple of the tile size (KParams::Wp)
    const int Wp = (Wd + kBlock - 1) / kBlock * kBlock;
    if ((long long)p.rows * Wp >= (1ll << 30)) return fail(PT_ERR_INVALID, "pt_init: frame too large (rows x padded width must stay below 2^30)");
    PTCHECK(checked_magic((uint32_t)Wd, k.magicW, k.shiftW));
    PTCHECK(set_tile_space(k, Wp, p.rows * Wp));
    k.ngeoms = in.ngeoms; k.nmats = in.nmats;
    // direct lighting: bounce `traceDepth` aims its diffuse scatter at a light and one more launch collects
    k.traceDepth = in.traceDepth + (in.direct() ? 1 : 0);
    k.directDepth = in.direct() ? in.traceDepth : 0;
    k.lensRadius = o.lens_radius;
    k.focalDistance = o.focal_distance;
    const H3 vn = hnormalize(H3{in.cam->view.x, in.cam->view.y, in.cam->view.z});
    k.viewN[0] = vn.x; k.viewN[1] = vn.y; k.viewN[2] = vn.z;
    p.dof = o.lens_radius > 0.0f;
    // plain: nothing in the scene takes the scatter's rarer branches (PT_AMD_NO_PLAIN: experiments / tests only)
    p.plain = !in.direct() && !(o.flags & PT_FLAG_MIXTURE_WEIGHTED) && !env_flag("PT_AMD_NO_PLAIN");
    for (int i = 0; i < in.nmats; ++i)
        if (in.mats[i].hasRefractive > 0.0f || (in.mats[i].hasReflective > 0.0f && in.mats[i].specularExponent > 0.0f)) p.plain = false;
    // ... and a path's material history fits one word: the PLAIN forms' pools carry one code of history_code_bits per scatter instead of the
    // throughput (ptk::PathPool), and traceDepth - 1 scatters lie behind a path that enters the last bounce.  A scene beyond that takes
    // the general forms: the same frame.
    if (history_code_bits(in.nmats) * (k.traceDepth - 1) > 32) p.plain = false;
    return PT_OK;
}

// The emitters of the direct-lighting bounce, file order: primitives with an emissive material, sampled through their unit cube -- and
// meshes (round 5) whose own or any of whose faces' materials emits, through the object-space bounds of their vertices
// (the CPU oracle restates this loop operation for operation: its rebuild_emitters)
// A scene with more emissive primitives than the table holds is refused under PT_FLAG_DIRECT_LIGHTING: choosing among the first kEmitMax alone
// is another estimator than the one the flag names (the oracle's, which chooses among all of them) -- a darker, differently lit frame.
int plan_emitters(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    k.nEmit = 0;
    if (in.o.flags & PT_FLAG_DIRECT_LIGHTING) {
        int emitting = 0;
        for (int i = 0; i < in.ngeoms; ++i)
            if (geom_emits(in, i) && (in.geoms[i].type != PT_MESH || (in.mesh_of(i) && in.mesh_of(i)->tris.size() >= 9))) ++emitting;
        if (emitting > kEmitMax)
            return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DIRECT_LIGHTING samples at most %d emissive primitives, the scene has %d", kEmitMax, emitting);
    }
    for (int i = 0; i < in.ngeoms && k.nEmit < kEmitMax; ++i) {
        float c[3] = {0.0f, 0.0f, 0.0f}, e[3] = {1.0f, 1.0f, 1.0f};
        if (in.geoms[i].type == PT_MESH) {
            const ptm::HostMesh *m = in.mesh_of(i);
            if (!m || m->tris.size() < 9) continue;
            float lo[3] = {m->tris[0], m->tris[1], m->tris[2]}, hi[3] = {lo[0], lo[1], lo[2]};
            for (size_t q = 0; q + 2 < m->tris.size(); q += 3)
                for (int a = 0; a < 3; ++a) {
                    lo[a] = lo[a] < m->tris[q + a] ? lo[a] : m->tris[q + a];
                    hi[a] = hi[a] < m->tris[q + a] ? m->tris[q + a] : hi[a];
                }
            for (int a = 0; a < 3; ++a) { c[a] = (lo[a] + hi[a]) * 0.5f; e[a] = hi[a] - lo[a]; }
        }
        if (!geom_emits(in, i)) continue;
        const PtVec3 sc = in.geoms[i].scale;
        const float sx = sc.x * e[0], sy = sc.y * e[1], sz = sc.z * e[2];
        k.emitRho2[k.nEmit] = ((sx * sx + sy * sy) + sz * sz) * 0.25f;
        for (int a = 0; a < 3; ++a) { k.emitBox[k.nEmit][a] = c[a]; k.emitBox[k.nEmit][3 + a] = e[a]; }
        k.emitGeom[k.nEmit++] = i;
    }
    return PT_OK;
}

// Path pools: a bounce's queue is kSeg = kCls x kSub segments, each a list of chunks handed out on demand, one ahead of
// their use (ptk::reserveRun).  At most nLocal * maxBatch paths are alive; every segment may end in a partly filled
// chunk and holds one chunk installed ahead: ceil(paths / chunk) + 2 kSeg chunks always suffice, whatever the
// distribution over the classes (+ the trash chunk 0).  Chunk size: a power of two, at least 2048 (rounds 1-3: ~1/1024 of the
// paths, so that the slack stayed around 10 % while a chunk outlasts the appends of one memory round trip).
int plan_pools(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    p.maxBatch = in.o.max_batch > 0 ? in.o.max_batch : 1;
    {   // a path carries pixelIndex | batch index << pixBits in ONE word (ptk::PathC)
        int pixBits = 1, batchBits = 0;
        while (((long long)k.W * k.H - 1) >> pixBits) ++pixBits;
        while ((p.maxBatch - 1) >> batchBits) ++batchBits;
        if (pixBits + batchBits > 32)
            return fail(PT_ERR_INVALID, "pt_init: %d x %d pixels and max_batch %d need %d + %d bits of a path's 32-bit index word: lower max_batch", k.W, k.H,
                        p.maxBatch, pixBits, batchBits);
        k.pixBits = pixBits;
    }
    if (p.maxBatch == 1) p.flags &= ~PT_FLAG_TRACE_AHEAD;   // nothing to trace ahead with: every call traces its own iteration
    // slots are 32-bit element indices with 32-bit byte offsets: paths per pool must stay below 2^30
    const long long maxPaths = (long long)p.nLocal * p.maxBatch;
    if (maxPaths > (1ll << 29)) return fail(PT_ERR_INVALID, "pt_init: max_batch x pixels too large (limit 2^29 paths per batch)");
    if ((long long)k.nLocalPad * p.maxBatch >= (1ll << 30))     // (the camera-ray tiles' index space: rows padded to the tile size)
        return fail(PT_ERR_INVALID, "pt_init: max_batch x rows x padded width too large (limit 2^30)");
    p.numTilesMax = (int)((maxPaths + kBlock - 1) / kBlock) + kSeg;
    // (round 4: ~1/256 of the paths, at most 2^18, where it was 1/1024 and 2^17 -- a run that opens a new chunk pays a dependent
    // look-up of the chunk list INSIDE the reservation's window, and four times fewer of them are +2 % on C2, +4 % on the closed box
    // (profiles/r04_chunk_size_sweep.txt); the slack of 2 kSeg chunks then doubles a mid-sized pool, which 288 GB shrug off)
    k.chunkShift = kMinChunkShift;
    while (k.chunkShift < 18 && (maxPaths >> k.chunkShift) > 256) ++k.chunkShift;
    if (const char *e = getenv("PT_AMD_CHUNK_SHIFT")) {      // experiments only
        const int v = atoi(e);
        if (v >= kMinChunkShift && v <= 20) k.chunkShift = v;
    }
    const long long chunkPaths = 1ll << k.chunkShift;
    p.poolChunks = (int)((maxPaths + chunkPaths - 1) / chunkPaths) + 2 * kSeg + 1;
    if (const char *e = getenv("PT_AMD_POOL_CHUNKS")) {      // tests only: an undersized pool must fail loudly (PT_ERR_DEVICE)
        const int v = atoi(e);
        if (v >= kSeg + 2) p.poolChunks = v;
    }
    k.poolChunks = p.poolChunks;
    p.poolCap = (size_t)p.poolChunks << k.chunkShift;
    // scenes with meshes: a record per path of a bounce's input queue (camera rays: per pixel of the tiles' padded index space) -- BounceArgs::meshHit
    bool anyMesh = false;
    for (int i = 0; i < in.ngeoms; ++i) anyMesh = anyMesh || in.geoms[i].type == PT_MESH;
    p.meshHitWords = anyMesh ? std::max(p.poolCap, (size_t)k.nLocalPad * (size_t)p.maxBatch) : 0;
    // Iterations are independent (RNG keyed on pixel/iteration/depth), so up to `nslots` of them are in flight
    // on their own streams; the small late-bounce launches of one overlap the big early launches of the next.
    p.nslots = in.o.pipeline_depth > 0 ? in.o.pipeline_depth : 3;
    return PT_OK;
}

// the primitives and the materials as the kernels read them; triangle meshes: one record array for the scene, a hierarchy per mesh (pt_mesh.h)
int plan_geoms(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const int ngeoms = in.ngeoms;
    p.hg.resize(ngeoms ? ngeoms : 1);
    p.hm.resize(in.nmats ? in.nmats : 1);
    const bool flatMeshes = env_flag("PT_AMD_MESH_FLAT");   // tests only: no hierarchy
    p.meshBox.resize(ngeoms ? ngeoms : 1);
    p.boxes.assign(ngeoms ? ngeoms : 1, nullptr);
    p.triBase.assign(ngeoms ? ngeoms : 1, 0u);
    for (int i = 0; i < ngeoms; ++i) {
        float *box = p.meshBox[i].data();
        const bool isMesh = in.geoms[i].type == PT_MESH;
        if (isMesh) p.boxes[i] = box;
        uint32_t root = ptd::kMeshEnd, stride = 0;
        const uint32_t unit0 = (uint32_t)p.meshRecs.size();      // (the mesh's units: its triangles -- and normals -- lie in [unit0, root))
        if (isMesh) {
            const ptm::HostMesh *m = in.mesh_of(i);
            for (int fm : m->mats)
                if (fm >= in.nmats) return fail(PT_ERR_INVALID, "pt_init: a face of mesh geom %d names material %d of %d", i, fm, in.nmats);
            const ptm::MeshLayout lay = ptm::appendMesh(m->tris.data(), (int)(m->tris.size() / 9), flatMeshes, p.meshRecs, box,
                                                        m->normals.empty() ? nullptr : m->normals.data(), m->mats.empty() ? nullptr : m->mats.data());
            root = lay.root;
            stride = lay.stride;
            p.meshStackNeed = std::max(p.meshStackNeed, lay.stackNeed);
            if (p.meshRecs.size() >= (1ull << 31)) return fail(PT_ERR_INVALID, "pt_init: too many triangles");
        }
        GeomDev &G = p.hg[i];
        pack_geom(in.geoms[i], G, k.pos, isMesh ? box : nullptr);
        G.meshRoot = root;
        if (isMesh) { G.meshStride = stride; G.meshUnit0 = unit0; G.meshUnit1 = root; p.triBase[i] = (unit0 + 3u) & ~3u; }
        if (in.geoms[i].type == PT_CUBE) {
            if (k.nCubes >= 32767) return fail(PT_ERR_INVALID, "pt_init: more than 32767 cubes");
            G.frameSlot = (short)k.nCubes++;
        }
    }
    for (int i = 0; i < in.nmats; ++i) pack_material(in.mats[i], p.hm[i]);
    p.mesh = !p.meshRecs.empty();
    return PT_OK;
}

// Camera rays: pixel rectangles, their union and the per-row lists (thin lens: none -- rays start anywhere on the lens).
// The camera-ray tiles' index space covers only the column bands (of kBlock pixels) and the rows of this shard that meet the
// scene rectangle: at 16:9 two of Cornell's five bands lie outside it, and a workgroup spent a tenth of the launch
// stepping over their tiles one by one.  The pixels never visited are misses whatever their jitter: tallied at once.
int plan_camera_cull(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const PtOptions &o = in.o;
    const int Wd = k.W, H = k.H, rows = p.rows;
    const CameraCull &cc = p.cc;
    const bool cullOff = p.dof || env_flag("PT_AMD_NO_CAMERA_CULL");   // (the variable: tests only)
    build_camera_cull(in.geoms, in.ngeoms, k, cullOff, p.boxes, p.hg, p.cc);
    for (int a = 0; a < 4; ++a) k.sceneRect[a] = cc.sceneRect[a];
    const int perRow = k.Wp / kBlock;
    int c0 = 0, c1 = perRow - 1, r0 = 0, r1 = rows - 1;
    if (cc.sceneRect[0] > cc.sceneRect[2] || cc.sceneRect[1] > cc.sceneRect[3]) {      // nothing can be hit
        c1 = -1; r1 = -1;
    } else {
        c0 = std::max(cc.sceneRect[0], 0) / kBlock;
        c1 = std::min(std::min(cc.sceneRect[2], Wd - 1) / kBlock, perRow - 1);
        // rows y = lr * shard_count + shard_rank inside [sceneRect[1], sceneRect[3]]
        const int y0 = std::max(cc.sceneRect[1], 0), y1 = std::min(cc.sceneRect[3], H - 1);
        r0 = y0 <= o.shard_rank ? 0 : (y0 - o.shard_rank + o.shard_count - 1) / o.shard_count;
        r1 = y1 < o.shard_rank ? -1 : std::min((y1 - o.shard_rank) / o.shard_count, rows - 1);
    }
    const int nCols = std::max(c1 - c0 + 1, 0), nRows = std::max(r1 - r0 + 1, 0);
    const long long visited = nCols > 0 && nRows > 0 ? (long long)nRows * (std::min(Wd, (c1 + 1) * kBlock) - c0 * kBlock) : 0;
    k.firstY0 = (nRows > 0 ? r0 : 0) * o.shard_count + o.shard_rank;      // (the first column: the band of sceneRect[0], k_bounce)
    k.firstSkipped = (int)((long long)p.nLocal - visited);
    const int Wp = std::max(nCols, 1) * kBlock;                   // (>= one band: the divisions stay defined)
    return set_tile_space(k, Wp, nCols > 0 ? nRows * Wp : 0);
}

// Small primitives the queue is binned by (k_bounce): the spheres when there are at most kBinMax of them, then the
// cubes whose bounding ball is small against the scene's (<= 0.3 of its radius), smallest first.  A choice that only
// steers which tiles skip which tests; results never depend on it.
void plan_bins(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const PtGeom *geoms = in.geoms;
    const int ngeoms = in.ngeoms;
    std::vector<GeomDev> &hg = p.hg;
    double cm[3] = {0, 0, 0}, sceneR = 0;
    for (int i = 0; i < ngeoms; ++i)
        for (int a = 0; a < 3; ++a) cm[a] += hg[i].centre[a] / std::max(ngeoms, 1);
    for (int i = 0; i < ngeoms; ++i) {
        const double dx = hg[i].centre[0] - cm[0], dy = hg[i].centre[1] - cm[1], dz = hg[i].centre[2] - cm[2];
        const double r = std::sqrt(dx * dx + dy * dy + dz * dz) + hg[i].boundR;
        if (std::isfinite(r)) sceneR = std::max(sceneR, r);
    }
    int nsph = 0;
    for (int i = 0; i < ngeoms; ++i) nsph += geoms[i].type == PT_SPHERE;
    std::vector<std::pair<double, int>> cand;
    for (int i = 0; i < ngeoms; ++i) {
        if (!std::isfinite(hg[i].cullR2)) continue;                       // never culled: cannot take part
        const double r = hg[i].boundR;
        if (geoms[i].type == PT_SPHERE) { if (nsph <= kBinMax) cand.emplace_back(-1.0, i); }   // spheres first
        else if (r <= 0.3 * sceneR) cand.emplace_back(r, i);
    }
    std::sort(cand.begin(), cand.end());
    k.nBinned = 0;
    for (size_t c = 0; c < cand.size() && k.nBinned < kBinMax; ++c) {
        k.binGeom[k.nBinned++] = cand[c].second;
        hg[cand[c].second].binned = 1;
        hg[cand[c].second].flags |= 2;
        hg[cand[c].second].cullFlags |= 2;
    }
    // Mesh scenes bin by two candidate bits (pt_trace.h: kClsMax): the costliest binned mesh (most triangles) alone in group 1 when there is
    // another binned primitive beside it, everything else in group 0 -- a tile of the next bounce then walks that mesh only when its paths
    // can hit it, with all its lanes, instead of every cand tile walking every mesh with some.
    if (p.mesh && k.nBinned > 1) {
        int bestB = -1;
        size_t bestTris = 0;
        for (int b = 0; b < k.nBinned; ++b)
            if (geoms[k.binGeom[b]].type == PT_MESH) {
                const size_t nt = in.mesh_of(k.binGeom[b])->tris.size() / 9;
                if (nt > bestTris) { bestTris = nt; bestB = b; }
            }
        if (bestB >= 0) p.binGroup[bestB] = 1;
    }
    // (PT_AMD_NO_TIGHT_CANDIDATES, tests only: no second condition, the classes are those of the bounding balls alone)
    const bool tight = !env_flag("PT_AMD_NO_TIGHT_CANDIDATES");
    for (int b = 0; b < kBinMax; ++b) {                      // (KParams::binCull: the binned primitives' culling groups, inline)
        for (int q = 0; q < 8; ++q) k.binCull[b][q] = k.binBox[b][q] = 0.0f;
        k.binCull[b][3] = -INFINITY;                          // beyond nBinned: certified for everybody
        if (b < k.nBinned) {
            const GeomDev &G = hg[k.binGeom[b]];
            k.binCull[b][0] = G.centre[0]; k.binCull[b][1] = G.centre[1]; k.binCull[b][2] = G.centre[2];
            k.binCull[b][3] = G.cullR2; k.binCull[b][4] = G.cullK;
            // word 5: the primitive's candidate bit in a survivor's class (k_bounce<..., MESH>): 1 = group 0, 2 = group 1
            const uint32_t bit = 1u << p.binGroup[b];
            memcpy(&k.binCull[b][5], &bit, sizeof bit);
            // word 6: the KIND of the second sufficient condition for the miss (KParams::binBox) -- 2 a sphere: the half-line; 1 a cube: the
            // slab certificate against its inflated world box, issued for origins within the bound wall_box states for that box.
            // The inflation is wall_box's for a SMALL cube as it is: delta = 4e-5 S with S >= the cube's largest |coordinate| and >= its
            // diagonal, while the reference's evaluation moves the boundary by ~2e-7 (|o| + S) whatever the cube's size or aspect -- the
            // object-space products of a thin axis are larger by the aspect and scaled back by it -- and |o| <= omax < 5 S bounds that by
            // 1.2e-6 S, a thirtieth of delta.  What a small cube changes is omax itself: an axis-aligned cube of extent 0.1 at the world's origin
            // has S = 0.17 and gets certificates for origins within 0.8 of it only (turned by 10 / 20 / 30 degrees, as
            // tests/test_candidate_certificates_cpu.py has it: S = 0.26, within 1.23); beyond the bound the ball alone decides.
            // (pt_test_wall_box_sweep sweeps thin, small and rotated cubes from touching them to 64 box sizes away.)
            int32_t kind = 0;
            WallBox wb;
            double om = 0;
            if (tight && geoms[k.binGeom[b]].type == PT_SPHERE) kind = 2;
            else if (tight && geoms[k.binGeom[b]].type == PT_CUBE && wall_box(geoms[k.binGeom[b]], wb, &om) >= 0 && om > 0) {
                kind = 1;
                for (int a = 0; a < 3; ++a) { k.binBox[b][a] = wb.lo[a]; k.binBox[b][3 + a] = wb.hi[a]; }
                k.binBox[b][6] = std::nextafter((float)om, 0.0f);
            }
            memcpy(&k.binCull[b][6], &kind, sizeof kind);
        }
    }
}

// Walls: the large cubes -- not binned, finite -- at most kWallMax of them, the largest first.  Survivors are classed by
// the one wall they can still hit (ptd::wallCertainMiss against the inflated world boxes computed here), so a tile of
// the next bounce tests one wall instead of all of them, and a survivor that can hit nothing at all ends at once.
// A choice that only steers which tiles skip which tests; results never depend on it.
void plan_walls(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    std::vector<GeomDev> &hg = p.hg;
    p.hw.resize(kWallMax);
    std::vector<int> wallGeom;
    choose_walls(in.geoms, in.ngeoms, hg, k, p.hw, wallGeom);
    // the walls' inner faces, in the wall table's own entries: a later tile whose list is one wall takes the face without the slab test
    // where every lane's certificate holds (k_bounce; PT_AMD_NO_WALL_RESOLVE, tests only: every wall -1)
    choose_wall_faces(in.geoms, k, wallGeom, env_flag("PT_AMD_NO_WALL_RESOLVE"), p.hw);
    for (int w = 0; w < k.nWalls; ++w) {
        hg[wallGeom[w]].flags |= (w + 1) << 2;
        hg[wallGeom[w]].cullFlags |= (w + 1) << 2;
    }
    if (env_flag("PT_AMD_NO_WALLS")) { for (int i = 0; i < in.ngeoms; ++i) { hg[i].flags &= 3; hg[i].cullFlags &= 3; } k.nWalls = 0; k.wallOMax = 0.0f; k.nSlotWalls = 0; k.nPlaneWalls = 0; }   // experiments only
    if (k.nPlaneWalls > 0) p.plain = false;      // (the rotated walls' certificate lives in the general instantiations only: k_bounce, wallPlanesOriented)
    k.allClassified = k.nWalls > 0 ? 1 : 0;
    for (int i = 0; i < in.ngeoms; ++i)
        if (!hg[i].binned && (hg[i].flags & 28) == 0) k.allClassified = 0;
    k.emittersBinned = k.nBinned > 0 ? 1 : 0;
    for (int i = 0; i < in.ngeoms; ++i)
        if (geom_emits(in, i) && !hg[i].binned) k.emittersBinned = 0;
}

// textured scenes: every texel one float4, the textures one after another; per primitive its TexGeom; per textured triangle two float4
int plan_textures(const SceneIn &in, ScenePlan &p) {
    p.bump = !in.bumpBindings.empty();
    p.tex = !in.texBindings.empty() || p.bump;
    if (!p.tex) return PT_OK;
    for (const HostTexture &t : in.textures) {
        p.texDesc.push_back(make_int4((int)p.texels.size(), t.w, t.h, 0));
        for (size_t q = 0; q < (size_t)t.w * t.h; ++q) p.texels.push_back(make_float4(t.rgb[3 * q], t.rgb[3 * q + 1], t.rgb[3 * q + 2], 0.0f));
    }
    p.texGeom.assign(in.ngeoms ? in.ngeoms : 1, ptd::TexGeom{-1, 0, 0, 0});
    for (int i = 0; i < in.ngeoms; ++i) p.texGeom[i].kind = in.geoms[i].type == PT_CUBE ? 1 : (in.geoms[i].type == PT_MESH ? 2 : 0);
    for (const HostTexBinding &b : in.texBindings) {
        ptd::TexGeom &g = p.texGeom[b.geom];
        g.tex = b.texture;
        if (b.uvs.empty()) continue;
        g.uvBase = (int)(p.texUV.size() / 2);
        g.triBase = (int)p.triBase[b.geom];
        pack_uvs(b.uvs, b.ntris, p.texUV);
        if (p.texUV.size() >= (1ull << 31)) return fail(PT_ERR_INVALID, "pt_init: too many textured triangles");
    }
    if (p.texUV.empty()) p.texUV.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    return PT_OK;
}

// bump-mapped scenes: per primitive its BumpGeom; per bumped triangle two float4 of corner UVs and two of tangents (a mesh's rows of its own,
// even where its texture binding carries the same UVs)
int plan_bump_maps(const SceneIn &in, ScenePlan &p) {
    if (!p.bump) return PT_OK;
    p.bumpGeom.assign(in.ngeoms ? in.ngeoms : 1, ptd::BumpGeom{-1, 0, 0, 0});
    for (const HostBumpBinding &b : in.bumpBindings) {
        ptd::BumpGeom &g = p.bumpGeom[b.geom];
        g.tex = b.texture;
        memcpy(&g.scaleBits, &b.scale, 4);
        if (b.uvs.empty()) continue;
        const ptm::HostMesh *m = in.mesh_of(b.geom);
        g.uvBase = (int)(p.bumpUV.size() / 2);
        g.triBase = (int)p.triBase[b.geom];
        pack_uvs(b.uvs, b.ntris, p.bumpUV);
        for (int f = 0; f < b.ntris; ++f) {
            float4 tu, tv;
            meshTangents(m->tris.data() + 9 * (size_t)f, b.uvs.data() + 6 * (size_t)f, tu, tv);
            p.bumpTan.push_back(tu);
            p.bumpTan.push_back(tv);
        }
        if (p.bumpUV.size() >= (1ull << 31)) return fail(PT_ERR_INVALID, "pt_init: too many bumped triangles");
    }
    if (p.bumpUV.empty()) { p.bumpUV.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f)); p.bumpTan.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f)); }
    return PT_OK;
}

// The SWEPT primitives of a scene with many small ones (round 5: cubes too -- rounds 2-4 swept spheres only, and 64 small cubes cost
// 4.7 x what 64 spheres did, profiles/r05_generality.txt): every sphere, and every cube that is neither a wall nor binned.  Their
// bounding balls are swept per lane from a packed table (ptk::SphereCull) instead of being visited one by one by the whole wave.
int plan_swept(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    std::vector<GeomDev> &hg = p.hg;
    const int ngeoms = in.ngeoms;
    p.swept.assign(ngeoms, 0);
    for (int i = 0; i < ngeoms; ++i) {
        const bool smallCube = in.geoms[i].type == PT_CUBE && !hg[i].binned && (hg[i].flags & 28) == 0 && std::isfinite(hg[i].cullR2);
        p.swept[i] = in.geoms[i].type == PT_SPHERE || smallCube;
        p.nswept += p.swept[i];
    }
    p.many = p.nswept > kBinMax;
    if (p.many && ngeoms > 65535) return fail(PT_ERR_INVALID, "pt_init: more than 65535 primitives");
    if (!p.many) std::fill(p.swept.begin(), p.swept.end(), 0);
    for (int i = 0; i < ngeoms; ++i)
        if (p.swept[i] && in.geoms[i].type == PT_CUBE) {
            p.sweptCubes = true;
            hg[i].flags |= 64;                        // (bit 6: a swept cube -- the camera-ray bounce lists it like a sphere)
            hg[i].cullFlags |= 64;
        }
    if (!p.many) return PT_OK;
    // the later bounces take the swept primitives from a packed copy of their culling data (ptk::SphereCull)
    std::vector<SphereCull> &sc = p.sc;
    for (int i = 0; i < ngeoms; ++i)
        if (p.swept[i]) {
            SphereCull e;
            memset(&e, 0, sizeof e);
            for (int a = 0; a < 3; ++a) e.centre[a] = hg[i].centre[a];
            e.cullR2 = hg[i].cullR2;
            e.cullK = hg[i].cullK + kUnitDirSlack;      // (the sweep's direction is normalised approximately: sphereHalfLineExcess)
            e.geom = i;
            sc.push_back(e);
        }
    // the K |oc|^2 term of the certificate folded into the sweep's direction (ptd::sphereHalfLineExcessScaled): one factor for the
    // scene, from its largest K, and every threshold multiplied by its square -- both rounded upwards (the conservative side)
    double kmax = 0.0;
    for (const SphereCull &e : sc) kmax = std::max(kmax, (double)e.cullK);
    const float sdir = std::nextafter((float)std::sqrt(1.0 / (1.0 - kmax)), INFINITY);
    k.sphDirScale = sdir;
    for (SphereCull &e : sc)
        if (std::isfinite(e.cullR2)) e.cullR2 = std::nextafter((float)((double)e.cullR2 * (double)sdir * (double)sdir), INFINITY);
    // two spatial CLUSTERS (scenes without meshes, whose second candidate bit is free): build_sphere_clusters
    k.sphN0 = 0; k.sphOMax = 0.0f;
    for (int g = 0; g < 2; ++g) for (int q = 0; q < 8; ++q) k.sphBox[g][q] = 0.0f;
    if (!p.mesh) {
        std::vector<int> binned(k.binGeom, k.binGeom + k.nBinned);
        build_sphere_clusters(in.geoms, ngeoms, hg, binned, sc, k.sphN0, k.sphOMax, k.sphBox);
    }
    if (k.sphOMax <= 0.0f) { k.sphN0 = 0; k.sphOMax = -1.0f; }      // no clusters: no certificate is issued, every tile sweeps the whole table
    else if (k.nWalls > 0) {
        // with the spheres behind candidate bits too, a survivor whose certificates leave no wall, no binned primitive and no cluster has
        // nothing left to hit (KParams::allClassified) -- when there is no primitive of another kind
        k.allClassified = 1;
        for (int i = 0; i < ngeoms; ++i)
            if (!hg[i].binned && (hg[i].flags & 28) == 0 && !p.swept[i]) k.allClassified = 0;
    }
    if (sc.size() % 2) sc.push_back(sc.back());      // (two per scalar load; testing a sphere twice changes nothing)
    // Hundreds of swept primitives (round 6): the flat sweep of the later bounces is linear in their number (512 spheres: 3.5 x the time of 64).
    // The table then comes in spatial groups of kSphGroupSize with a bounding ball each, and the later bounces take instantiations of their
    // own (k_bounce<..., GROUPS>: two-level sweep, no scene table in LDS).  PT_AMD_GROUPS=0 / 1: never / whenever possible (experiments, tests).
    k.nSphGroups = 0; k.grpN0 = 0; k.grpOMax = 0.0f; k.grpLds = 0;
    const char *ge = getenv("PT_AMD_GROUPS");
    // (textured scenes never: the grouped sweep is the ungrouped one's result, bit for bit, and the TEX forms leave it out)
    p.grouped = !p.mesh && !p.tex && (ge ? atoi(ge) != 0 : p.nswept >= kGroupedMin);
    if (p.grouped) {
        int n0 = k.sphN0;
        const double ob = scene_origin_bound(in.geoms, ngeoms, hg);
        build_sphere_groups(sc, n0, ob, sdir, p.groups, k.grpN0);
        k.sphN0 = n0;
        k.nSphGroups = (int)(sc.size() / (size_t)kSphGroupSize);
        k.grpOMax = std::nextafter((float)ob, 0.0f);
        k.grpLds = (int)sc.size() <= kGroupLdsMax ? 1 : 0;
    }
    k.nSphCull = (int)sc.size();
    return PT_OK;
}

// The per-primitive hit records, ready-made: a workgroup's prologue copies them to LDS in one round trip instead of following
// primitive -> material index -> material on the device (every workgroup of every launch did).
// Sphere-heavy scenes: the tables a workgroup stages in LDS -- the compact hit records, the cubes' face frames, the spheres' matrix rows,
// the sweep's entry -> primitive map -- as ONE image in the kernel's own layout (many_lds), so that the prologue is a straight copy of
// 16-byte words: gathering them field by field from the primitives took ~30 dependent round trips, 28 us at the head of every launch
// of C5 (profiles/timeline_phases.py: 62 k cycles against Cornell's 10 k).
void plan_hit_records(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const int ngeoms = in.ngeoms, nmats = in.nmats;
    if (!p.many) {
        p.geomHit.assign(p.hg.size() * sizeof(GeomHitDev), 0);
        GeomHitDev *hh = reinterpret_cast<GeomHitDev *>(p.geomHit.data());
        for (size_t i = 0; i < p.hg.size(); ++i) {
            GeomHitDev &h = hh[i];
            const GeomDev &G = p.hg[i];
            const int mi = (int)i < ngeoms && G.material >= 0 && G.material < nmats ? G.material : 0;
            const MaterialDev &M = p.hm[(size_t)mi];
            h.type = G.type;
            h.emittance = M.emittance; h.hasReflective = M.hasReflective; h.hasRefractive = M.hasRefractive;
            for (int a = 0; a < 3; ++a) h.color[a] = M.color[a];
            h.material = G.material;
            memcpy(h.nm, G.invT, sizeof h.nm);
            memcpy(h.cubeFrame, G.cubeFrame, sizeof h.cubeFrame);
        }
        return;
    }
    // (scenes of hundreds of primitives: the matrix rows -- 112 B per primitive -- stay in global memory, KParams::ldsRowFloats = 0; with
    // them a workgroup of the 518-primitive scene took 103 KB of LDS, one per CU.  The limit: what four workgroups per CU leave each.)
    const int rowFloatsAll = ngeoms * kSphRowFloats;
    const size_t ldsWithRows = lds_head(nmats, kClsMax) + many_lds(ngeoms, k.nCubes, rowFloatsAll, k.nSphCull).tables() + (size_t)kListMax * kBlock * sizeof(uint16_t);
    const bool rowsInLds = ldsWithRows <= 40 * 1024 && !p.grouped && !env_flag("PT_AMD_ROWS_GLOBAL");   // (the variable: tests only)
    k.ldsRowFloats = rowsInLds ? rowFloatsAll : 0;
    const ManyLds L = many_lds(ngeoms, k.nCubes, k.ldsRowFloats, k.nSphCull);
    // (+ 64 bytes: behind the last cube's frames a row of NaNs -- what k_bounce<..., GROUPS>, which reads the frames from this image in
    // global memory, selects for a cube hit without an exit slab, as the other kernels select their NaN row in LDS)
    std::vector<unsigned char> &blob = p.geomHit;
    blob.assign(L.tables() + L.map + 64, 0);
    p.rowsGlobal.assign(rowsInLds ? 0 : (size_t)rowFloatsAll, 0.0f);
    GeomHitSmall *hs = reinterpret_cast<GeomHitSmall *>(blob.data());
    float *fr = reinterpret_cast<float *>(blob.data() + L.hit);
    float *rows = rowsInLds ? reinterpret_cast<float *>(blob.data() + L.hit + L.frames) : p.rowsGlobal.data();
    uint16_t *map = reinterpret_cast<uint16_t *>(blob.data() + L.tables());
    for (int g = 0; g < ngeoms; ++g) {
        const GeomDev &G = p.hg[g];
        memcpy(hs[g].nm, G.invT, sizeof hs[g].nm);
        hs[g].material = G.material; hs[g].type = G.type; hs[g].frame = G.type == 1 ? (int)G.frameSlot : 0;
        if (G.type == 1) memcpy(fr + (size_t)G.frameSlot * 54, G.cubeFrame, 54 * sizeof(float));
        float *r = rows + (size_t)g * kSphRowFloats;
        memcpy(r, G.inv, 12 * sizeof(float)); memcpy(r + 12, G.xf, 12 * sizeof(float)); memcpy(r + 24, G.invZ, 3 * sizeof(float));
    }
    for (int i = 0; i < k.nSphCull; ++i) map[i] = (uint16_t)p.sc[i].geom;
    if (p.grouped) {
        const float qnan = std::nanf("");
        for (int q = 0; q < 9; ++q) memcpy(blob.data() + L.hit + (size_t)k.nCubes * 54 * sizeof(float) + q * sizeof(float), &qnan, sizeof qnan);
    }
}

// Later bounces: which primitives a tile of queue class c looks at.  Class bit 3 = its paths may hit a binned primitive;
// bits 0-2 in a scene with walls = the one wall they can still hit (6: any, 7: none), else the direction octant.
void plan_classes(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    std::vector<int> &idx = p.classIdx;
    const int ncls = (p.mesh || p.many) ? kClsMax : kCls;                 // (mesh and sphere-heavy scenes: two candidate bits, 32 classes)
    for (int c = 0; c < kClsMax; ++c) {
        k.classOff[c] = (int)idx.size();
        if (c >= ncls) continue;
        const int small = c >> 3;                                          // candidate bits: which groups of binned primitives
        const int wall = k.nWalls > 0 ? (c & 7) : 6;
        for (int i = 0; i < in.ngeoms; ++i) {
            if (p.swept[i]) continue;                                        // swept from their packed culling data
            if (p.hg[i].binned) {
                int grp = 0;
                for (int b = 0; b < k.nBinned; ++b)
                    if (k.binGeom[b] == i) grp = p.binGroup[b];
                if (!((small >> grp) & 1)) continue;
            }
            const int w = (p.hg[i].flags >> 2) & 7;                        // 1 + index among the walls, 0: not one
            if (w != 0 && wall != 6 && w != wall + 1) continue;
            idx.push_back(i);
        }
    }
    k.classOff[kClsMax] = (int)idx.size();
    if (idx.empty()) idx.push_back(0);
}

// Camera rays: where the camera-ray instantiation can take it (pinhole, no meshes -- their walk shares the row bands' index space,
// BounceArgs::meshHit -- and not the sphere-heavy one), the packed work list in place of the row bands: the tiles' index space of
// one iteration is then the list (KParams::nLocalPad), and every pixel outside it is tallied at once (KParams::firstSkipped)
int plan_camera_list(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const bool listOff = env_flag("PT_AMD_NO_CAMERA_LIST");   // (the variable: tests only)
    // the waves' face certificates (camera_face_certificate), where the instantiation reads them: not the textured forms
    // (PT_AMD_NO_CAMERA_RESOLVE, tests only: the same list, every wave unresolved)
    CameraResolve cr;
    const bool resolve = !listOff && !p.dof && !p.mesh && !p.many && !p.tex;
    if (resolve) {
        build_camera_resolve(in.geoms, in.ngeoms, k, p.hg, cr);
        cr.off = env_flag("PT_AMD_NO_CAMERA_RESOLVE");
    }
    bool built = false;
    if (!listOff && !p.dof && !p.mesh && !p.many) {
        if (resolve && in.faces) {       // the two passes, the certificates between them where the caller says
            CameraGroups G;
            built = camera_list_groups(p.cc, k.W, k.H, in.o.shard_rank, in.o.shard_count, k.nLocalPad, G);
            if (built) {
                PTCHECK(in.faces(G, cr));
                camera_list_emit(G, k.nLocalPad, p.cl, &cr);
            }
        } else {
            built = build_camera_list(p.cc, k.W, k.H, in.o.shard_rank, in.o.shard_count, k.nLocalPad, p.cl, resolve ? &cr : nullptr);
        }
    }
    if (built && !p.cl.pix.empty()) {
        k.firstSkipped = (int)((long long)p.nLocal - p.cl.listed);
        return set_tile_space(k, k.Wp, (int)p.cl.pix.size());
    }
    p.cl = CameraList();
    return PT_OK;
}

// The mesh walks (k_mesh_walk) look at the meshes alone: the classes' lists, one list of all, the rows' lists (pairs as rowIdx's);
// their rows, one per mesh in the order of the meshes' ordinals (ptk::WalkMesh)
int plan_walks(const SceneIn &in, ScenePlan &p) {
    if (!p.mesh) return PT_OK;
    const KParams &k = p.prm;
    std::vector<GeomDev> &hg = p.hg;
    std::vector<int> &w = p.walkIdx;
    const std::vector<int> &idx = p.classIdx;
    for (int c = 0; c < kClsMax; ++c) {
        p.walkClassOff[c] = (int)w.size();
        for (int e = k.classOff[c]; e < k.classOff[c + 1]; ++e)
            if (hg[idx[e]].flags & 32) w.push_back(idx[e]);
    }
    p.walkClassOff[kClsMax] = (int)w.size();
    p.walkAll0 = (int)w.size();
    for (int i = 0; i < in.ngeoms; ++i)
        if (hg[i].flags & 32) {
            if (w.size() - (size_t)p.walkAll0 >= 32767) return fail(PT_ERR_INVALID, "pt_init: more than 32767 meshes");
            hg[i].frameSlot = (short)(w.size() - (size_t)p.walkAll0);     // (a mesh's ordinal: its row of the walk's LDS table)
            w.push_back(i);
        }
    p.walkAll1 = (int)w.size();
    const int nm = p.walkAll1 - p.walkAll0;
    p.walkMeshRows.resize((size_t)nm);
    for (int q = 0; q < nm; ++q) {
        const GeomDev &G = hg[(size_t)w[(size_t)p.walkAll0 + q]];
        WalkMesh &r = p.walkMeshRows[(size_t)q];
        memcpy(r.inv, G.inv, sizeof r.inv); memcpy(r.invZ, G.invZ, sizeof r.invZ);
        r.root = G.meshRoot;
        memcpy(r.xf, G.xf, sizeof r.xf); memcpy(r.camObj, G.camObj, sizeof r.camObj);
        r.stride = G.meshStride;
    }
    const bool forceGlobal = env_flag("PT_AMD_WALK_ROWS_GLOBAL");      // tests only
    p.walkMeshLds = (nm <= kWalkMeshLdsMax && !forceGlobal) ? nm : 0;
    const CameraCull &cc = p.cc;
    if (!cc.rowOff.empty()) {
        if (w.size() % 2) w.push_back(0);                  // (the rows' entries are pairs: offsets count pairs from the array's start)
        std::vector<int> &ro = p.walkRowOff;
        ro.resize(cc.rowOff.size());
        for (size_t y = 0; y + 1 < cc.rowOff.size(); ++y) {
            ro[y] = (int)(w.size() / 2);
            for (int e = cc.rowOff[y]; e < cc.rowOff[y + 1]; ++e)
                if (hg[cc.rowIdx[2 * e]].flags & 32) { w.push_back(cc.rowIdx[2 * e]); w.push_back(cc.rowIdx[2 * e + 1]); }
        }
        ro[cc.rowOff.size() - 1] = (int)(w.size() / 2);
    }
    return PT_OK;
}

// the dynamic LDS of the launches, and what has to fit it
int plan_lds(const SceneIn &in, ScenePlan &p) {
    KParams &k = p.prm;
    const int nmats = in.nmats;
    const ManyLds L = many_lds(in.ngeoms, k.nCubes, k.ldsRowFloats, k.nSphCull);
    const size_t ldsFixed = lds_head(nmats, (p.mesh || p.many) ? kClsMax : kCls) + (p.many ? L.tables() : sizeof(GeomHitDev) * in.ngeoms);
    // (sphere-heavy scenes: the camera-ray launch keeps the lanes' candidate lists behind the tables, the later ones only the sweep's
    // entry -> primitive map -- 4 KB less, which is what their seventh workgroup per CU needs)
    // (... and, behind the map, the pooled pass's pair descriptors: [kWaves][64] words)
    const size_t listBytes = (size_t)kListMax * kBlock * sizeof(uint16_t), pairBytes = (size_t)kBlock * sizeof(uint32_t);
    k.pairOff = (int)(ldsFixed + L.map);
    p.ldsBytes = ldsFixed + (p.many ? std::max(listBytes, L.map + pairBytes) : 0);
    p.ldsBytesNext = (p.many && !p.mesh) ? ldsFixed + L.map + pairBytes : 0;
    if (p.grouped && !p.dof)      // (the camera-ray bounce of a grouped scene: the materials and the lanes' candidate lists)
        p.ldsBytes = lds_head(nmats, kClsMax) + listBytes + 16;
    if (p.grouped) {      // (the later bounces stage the materials and nothing else of the scene ...
        // ... and, behind them, the lanes' parked candidates: KParams::pairOff, [kCandPairs][kBlock] words)
        const size_t members = lds_head(nmats, kClsMax) + (k.grpLds ? ((size_t)k.nSphCull * 18 + 15) / 16 * 16 : 0);
        k.pairOff = (int)members;
        p.ldsBytesNext = members + (size_t)kCandPairs * kBlock * sizeof(uint32_t) + 16;
    }
    k.meshStackOff = 0;
    if (p.mesh) {        // (the lanes' stacks of far children belong to the walk's own launches: k_mesh_walk)
        p.ldsWalk = walkLdsBytes(p.meshStackNeed, p.walkMeshLds);
        if (p.ldsWalk > 160 * 1024) return fail(PT_ERR_INVALID, "pt_init: a mesh's hierarchy needs %d stack levels (%zu B of LDS for the lanes' stacks)", p.meshStackNeed, p.ldsWalk);
        // (the display filter launches k_gbuffer from pt_iterate: what ensure_guides would refuse there is refused here, with its message)
        if ((p.flags & PT_FLAG_DISPLAY_FILTER) && guideStackBytes(true, p.meshStackNeed) > 64 * 1024)
            return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DISPLAY_FILTER: guide buffers: a mesh hierarchy needs %d stack levels", p.meshStackNeed);
        // (... and so does k_albedo, whose lanes walk the meshes with k_gbuffer's stacks)
        if ((p.flags & PT_FLAG_DEMODULATE) && guideStackBytes(true, p.meshStackNeed) > 64 * 1024)
            return fail(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMODULATE: guide buffers: a mesh hierarchy needs %d stack levels", p.meshStackNeed);
    }
    if (p.ldsBytesNext == 0) p.ldsBytesNext = p.ldsBytes;
    if (p.ldsBytes > 160 * 1024) return fail(PT_ERR_INVALID, "pt_init: scene does not fit the 160 KiB LDS (%zu B)", p.ldsBytes);
    if (nmats >= 4096) return fail(PT_ERR_INVALID, "pt_init: more than 4095 materials");      // (TileArgs::hot holds nmats in 12 bits)
    return PT_OK;
}

// PT_OK, or what fail() returned: the scene is refused, and nothing but `p` has been touched
int plan_scene(const SceneIn &in, ScenePlan &p) {
    PTCHECK(check_scene(in));
    PTCHECK(plan_frame(in, p));
    PTCHECK(plan_emitters(in, p));
    PTCHECK(plan_pools(in, p));
    PTCHECK(plan_geoms(in, p));
    PTCHECK(plan_camera_cull(in, p));
    plan_bins(in, p);
    plan_walls(in, p);
    PTCHECK(plan_textures(in, p));
    PTCHECK(plan_bump_maps(in, p));
    PTCHECK(plan_swept(in, p));
    plan_hit_records(in, p);
    plan_classes(in, p);
    PTCHECK(plan_camera_list(in, p));
    PTCHECK(plan_walks(in, p));
    // the pools are history-coded exactly where the later bounces take the PLAIN form (pt_api.hip: bounce_form; pt_init checks the two agree)
    p.prm.histBits = (p.plain && !p.tex && !p.mesh && !p.many) ? history_code_bits(in.nmats) : 0;
    return plan_lds(in, p);
}
