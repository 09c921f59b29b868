// scene.cpp -- parser for the reference's scene-file format (reference src/scene.cpp:7-182), quirks kept:
//   * MATERIAL / OBJECT ids must be sequential, otherwise the block is skipped with an ERROR line (:37,:149)
//   * a MATERIAL block is exactly 7 lines, a CAMERA block 5 lines + EYE/VIEW/UP lines up to a blank line
//   * the object type line must be exactly "sphere" or "cube" (:48-53); TRANS/ROTAT/SCALE up to a blank line
//   * README.md:236 names a third object type, "mesh", which the reference's loader does not know: here the type line
//     `mesh <file.obj>` (path relative to the scene file) loads a Wavefront OBJ into Scene::meshes (loadObj below)
//   * the specular exponent keyword is SPECEX (:164) although the README says SPECX
//   * CRLF / CR / LF line ends; '//' comment lines are simply unknown keywords
//   * `TEXTURE <file>` in an OBJECT block (next to TRANS / ROTAT / SCALE; path relative to the scene file) binds an image texture to the
//     object (loadTexture); the reference's loader skips the unknown keyword, so a textured scene still loads there, untextured
//   * `BUMP <file> <scale>` likewise binds a height map (any texture file; channel 0) and its scale: the files are shared with TEXTURE by
//     resolved path; a missing or non-finite scale fails the load; the reference's loader skips this keyword too
//   * `TRANS_END`, `ROTAT_END`, `SCALE_END` (three floats each) in an OBJECT block give the object's pose at shutter close: Scene::stepGeoms
//     (scene.h) then holds the scene in 16 poses across the shutter; the reference's loader skips these keywords too, so such a file still
//     loads there, unmoved
// Unlike the reference, fields whose keyword is missing are zero instead of uninitialised.
#include "scene.h"

#include "pt_amd.h"

#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <stdexcept>

using utilityCore::safeGetline;
using utilityCore::tokenizeString;

namespace {
typedef std::vector<std::string> Tokens;
bool key(const Tokens &t, const char *k) { return !t.empty() && t[0] == k; }
float num(const Tokens &t, size_t i) { return i < t.size() ? (float)atof(t[i].c_str()) : 0.0f; }
lin::vec3 triple(const Tokens &t) { return lin::vec3(num(t, 1), num(t, 2), num(t, 3)); }

// Wavefront OBJ -> triangle soup.  `v x y z` and `f a b c ...` with a = i, i/j, i//k or i/j/k (1-based; negative = relative
// to the vertices read so far); polygons are fanned from their first vertex.  `vn x y z` + the third field of a face corner give
// vertex normals: kept only when EVERY corner of EVERY face names one (else the mesh is shaded flat).  `usemtl <k>` (k an integer
// = a MATERIAL of the scene file) gives the faces that follow a material of their own; any other name returns to the object's.
// `vt u v` + the second field of a face corner give texture coordinates, kept by the same all-or-nothing rule as the normals.
// Every other statement is ignored.
bool loadObj(const std::string &path, std::vector<float> &tris, std::vector<float> &normalsOut, std::vector<int> &matsOut,
             std::vector<float> &uvsOut) {
    std::ifstream fp(path.c_str());
    if (!fp.is_open()) return false;
    std::vector<float> verts, vnorm, normals, vtex, uvs;
    std::vector<int> mats;
    bool allNormals = true, anyMat = false, allUvs = true;
    int curMat = -1;
    std::string line;
    while (std::getline(fp, line)) {
        std::istringstream ss(line);
        std::string keyword;
        if (!(ss >> keyword)) continue;
        if (keyword == "v" || keyword == "vn") {
            double c[3] = {0, 0, 0};
            ss >> c[0] >> c[1] >> c[2];
            std::vector<float> &dst = keyword == "v" ? verts : vnorm;
            for (int a = 0; a < 3; ++a) dst.push_back((float)c[a]);
        } else if (keyword == "vt") {
            double c[2] = {0, 0};
            ss >> c[0] >> c[1];
            for (int a = 0; a < 2; ++a) vtex.push_back((float)c[a]);
        } else if (keyword == "usemtl") {
            std::string tok;
            curMat = -1;
            if (ss >> tok) {
                char *end = nullptr;
                const long k = strtol(tok.c_str(), &end, 10);
                if (end && *end == 0 && k >= 0 && k < 1000000) curMat = (int)k;
            }
        } else if (keyword == "f") {
            const int nv = (int)(verts.size() / 3), nn = (int)(vnorm.size() / 3), nt = (int)(vtex.size() / 2);
            std::vector<int> corner, ncorner, tcorner;
            std::string ref;
            bool ok = true;
            while (ss >> ref) {
                const int i = atoi(ref.c_str());              // (reads up to the first '/')
                const int k = i > 0 ? i - 1 : nv + i;
                if (i == 0 || k < 0 || k >= nv) { ok = false; break; }
                corner.push_back(k);
                int nk = -1;                                   // the normal: the field behind the second '/'
                const size_t s1 = ref.find('/');
                const size_t s2 = s1 == std::string::npos ? std::string::npos : ref.find('/', s1 + 1);
                if (s2 != std::string::npos && s2 + 1 < ref.size()) {
                    const int j = atoi(ref.c_str() + s2 + 1);
                    const int q = j > 0 ? j - 1 : nn + j;
                    if (j != 0 && q >= 0 && q < nn) nk = q;
                }
                ncorner.push_back(nk);
                int tk = -1;                                   // the texture coordinate: the field between the two '/'
                if (s1 != std::string::npos && s1 + 1 < ref.size() && ref[s1 + 1] != '/') {
                    const int j = atoi(ref.c_str() + s1 + 1);
                    const int q = j > 0 ? j - 1 : nt + j;
                    if (j != 0 && q >= 0 && q < nt) tk = q;
                }
                tcorner.push_back(tk);
            }
            for (size_t k = 2; ok && k < corner.size(); ++k) {
                const int tri[3] = {corner[0], corner[k - 1], corner[k]};
                const int ntri[3] = {ncorner[0], ncorner[k - 1], ncorner[k]};
                const int ttri[3] = {tcorner[0], tcorner[k - 1], tcorner[k]};
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 2; ++a) uvs.push_back(ttri[c] >= 0 ? vtex[2 * (size_t)ttri[c] + a] : 0.0f);
                if (ttri[0] < 0 || ttri[1] < 0 || ttri[2] < 0) allUvs = false;
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) {
                        tris.push_back(verts[3 * (size_t)tri[c] + a]);
                        normals.push_back(ntri[c] >= 0 ? vnorm[3 * (size_t)ntri[c] + a] : 0.0f);
                    }
                if (ntri[0] < 0 || ntri[1] < 0 || ntri[2] < 0) allNormals = false;
                mats.push_back(curMat);
                if (curMat >= 0) anyMat = true;
            }
        }
    }
    if (allNormals && !tris.empty()) normalsOut = normals; else normalsOut.clear();
    if (anyMat) matsOut = mats; else matsOut.clear();
    if (allUvs && !tris.empty()) uvsOut = uvs; else uvsOut.clear();
    return true;
}

// PPM / PFM header tokens: whitespace-separated, '#' starts a comment up to the line's end (PPM)
bool headerToken(std::istream &in, std::string &tok) {
    tok.clear();
    int c;
    while ((c = in.get()) != EOF) {
        if (c == '#' && tok.empty()) {
            while ((c = in.get()) != EOF && c != '\n' && c != '\r') {}
            continue;
        }
        if (isspace(c)) {
            if (!tok.empty()) return true;
            continue;
        }
        tok.push_back((char)c);
    }
    return !tok.empty();
}
int headerInt(std::istream &in) {
    std::string t;
    if (!headerToken(in, t)) return -1;
    char *end = nullptr;
    const long v = strtol(t.c_str(), &end, 10);
    return (end && *end == 0 && v >= 0 && v <= (1l << 30)) ? (int)v : -1;
}

}  // namespace

Texture loadTexture(const std::string &path) {
    std::ifstream in(path.c_str(), std::ios::binary);
    if (!in.is_open()) throw std::runtime_error("cannot read texture " + path);
    std::string magic;
    headerToken(in, magic);
    Texture t;
    t.path = path;
    const bool ppm = magic == "P3" || magic == "P6", pfm = magic == "PF" || magic == "Pf";
    if (!ppm && !pfm) throw std::runtime_error("texture " + path + ": not a PPM (P3 / P6) or PFM (PF / Pf) file");
    t.width = headerInt(in);
    t.height = headerInt(in);
    if (t.width < 1 || t.height < 1 || (long long)t.width * t.height > (1ll << 28))
        throw std::runtime_error("texture " + path + ": bad size");
    const size_t n = (size_t)t.width * t.height;
    t.rgb.resize(3 * n);
    if (ppm) {
        if (headerInt(in) != 255) throw std::runtime_error("texture " + path + ": only 8-bit PPM (maxval 255) is read");
        for (size_t i = 0; i < 3 * n; ++i) {
            int b;
            if (magic == "P6") {
                b = in.get();                                    // (the header's single whitespace byte was consumed with maxval)
                if (b == EOF) throw std::runtime_error("texture " + path + ": truncated");
            } else {
                b = headerInt(in);
                if (b < 0 || b > 255) throw std::runtime_error("texture " + path + ": bad sample");
            }
            t.rgb[i] = (float)b / 255.0f;
        }
    } else {
        std::string scale;
        if (!headerToken(in, scale)) throw std::runtime_error("texture " + path + ": truncated");
        const bool little = atof(scale.c_str()) < 0.0;           // (PFM: a negative scale = little-endian samples)
        const int ch = magic == "PF" ? 3 : 1;
        std::vector<unsigned char> raw(4 * (size_t)ch * n);
        if (!in.read(reinterpret_cast<char *>(raw.data()), (std::streamsize)raw.size())) throw std::runtime_error("texture " + path + ": truncated");
        for (size_t i = 0; i < (size_t)ch * n; ++i) {
            const unsigned char *b = raw.data() + 4 * i;
            const uint32_t w = little ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24
                                      : (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24;
            float f;
            memcpy(&f, &w, 4);
            // PFM stores its rows bottom to top: sample i of file row r is texel row height - 1 - r
            const size_t px = i / ch, r = px / t.width, x = px % t.width;
            const size_t dst = ((size_t)(t.height - 1 - r) * t.width + x) * 3;
            if (ch == 3) t.rgb[dst + i % 3] = f;
            else t.rgb[dst] = t.rgb[dst + 1] = t.rgb[dst + 2] = f;     // (Pf: one grey sample per texel)
        }
    }
    return t;
}

namespace {
void deriveFov(Camera &camera, float fovy) {
    // reference src/scene.cpp:133-136
    float yscaled = std::tan(fovy * (PI / 180));
    float xscaled = (yscaled * camera.resolution.x) / camera.resolution.y;
    float fovx = (std::atan(xscaled) * 180) / PI;
    camera.fov.x = fovx;
    camera.fov.y = fovy;
}
}  // namespace

Scene::Scene(std::string filename, bool verbose_) : verbose(verbose_) {
    if (verbose) std::cout << "Reading scene from " << filename << " ..." << std::endl << " " << std::endl;
    state.iterations = 0;
    state.traceDepth = 0;
    state.camera.resolution.x = state.camera.resolution.y = 0;
    state.camera.fov.x = state.camera.fov.y = 0.0f;
    {
        const size_t slash = filename.find_last_of('/');
        dir = slash == std::string::npos ? std::string() : filename.substr(0, slash + 1);
    }
    fp_in.open(filename.c_str());
    if (!fp_in.is_open()) {
        std::cout << "Error reading from file - aborting!" << std::endl;
        throw std::runtime_error("Error reading from file - aborting!");
    }
    std::string line;
    while (fp_in.good()) {
        safeGetline(fp_in, line);
        if (line.empty()) continue;
        const Tokens tokens = tokenizeString(line);
        bool block = true;
        if (tokens.size() >= 2 && key(tokens, "MATERIAL")) loadMaterial(tokens[1]);
        else if (tokens.size() >= 2 && key(tokens, "OBJECT")) loadGeom(tokens[1]);
        else if (key(tokens, "CAMERA")) loadCamera();
        else block = false;
        if (block && verbose) std::cout << " " << std::endl;
    }
    // `usemtl <k>` names a MATERIAL of THIS file.  An OBJ from elsewhere may carry numeric material names of its own: an index the
    // scene does not have falls back to the object's material, loudly (it used to surface only later, as pt_init's PT_ERR_INVALID).
    for (size_t i = 0; i < meshes.size(); ++i) {
        size_t bad = 0;
        for (size_t f = 0; f < meshes[i].mats.size(); ++f)
            if (meshes[i].mats[f] >= (int)materials.size()) {
                meshes[i].mats[f] = -1;
                ++bad;
            }
        if (bad)
            std::cout << "WARNING: mesh of object " << meshes[i].geom << ": " << bad << " faces name a material (usemtl <k>) the scene has "
                      << "not (" << materials.size() << " MATERIAL blocks): they take the object's material" << std::endl;
    }
    // a textured mesh needs texture coordinates on every corner (`vt`): without them the scene cannot be rendered
    geomTextures.resize(geoms.size(), -1);
    for (size_t i = 0; i < meshes.size(); ++i)
        if (geomTextures[meshes[i].geom] >= 0 && meshes[i].uvs.empty()) {
            std::cout << "ERROR: object " << meshes[i].geom << " is textured and its mesh has no texture coordinates - aborting!" << std::endl;
            throw std::runtime_error("textured mesh without texture coordinates");
        }
    // ... and so does a bump-mapped one
    geomBumps.resize(geoms.size(), -1);
    bumpScales.resize(geoms.size(), 0.0f);
    for (size_t i = 0; i < meshes.size(); ++i)
        if (geomBumps[meshes[i].geom] >= 0 && meshes[i].uvs.empty()) {
            std::cout << "ERROR: object " << meshes[i].geom << " is bump-mapped and its mesh has no texture coordinates - aborting!" << std::endl;
            throw std::runtime_error("bump-mapped mesh without texture coordinates");
        }
    buildStepGeoms();
}

void Scene::buildStepGeoms() {
    static_assert(kMotionSteps == PT_MOTION_STEPS, "scene.h and include/pt_amd.h name one number of steps");
    bool any = false;
    for (const PoseEnd &e : poseEnds) any = any || e.trans || e.rotat || e.scale;
    if (!any) return;
    const auto lerp = [](const lin::vec3 &a, const lin::vec3 &b, float t) {
        return lin::vec3(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t);
    };
    stepGeoms.reserve((size_t)kMotionSteps * geoms.size());
    for (int s = 0; s < kMotionSteps; ++s) {
        const float t = ((float)s + 0.5f) / (float)kMotionSteps;
        for (size_t i = 0; i < geoms.size(); ++i) {
            Geom g = geoms[i];
            const PoseEnd e = i < poseEnds.size() ? poseEnds[i] : PoseEnd();
            if (e.trans) g.translation = lerp(geoms[i].translation, e.t, t);
            if (e.rotat) g.rotation = lerp(geoms[i].rotation, e.r, t);
            if (e.scale) g.scale = lerp(geoms[i].scale, e.s, t);
            if (e.trans || e.rotat || e.scale) {
                g.transform = utilityCore::buildTransformationMatrix(g.translation, g.rotation, g.scale);
                g.inverseTransform = lin::inverse(g.transform);
                g.invTranspose = lin::inverseTranspose(g.transform);
            }
            stepGeoms.push_back(g);
        }
    }
}

int Scene::textureIndex(const std::string &path) {
    for (size_t j = 0; j < textures.size(); ++j)
        if (textures[j].path == path) return (int)j;
    try {
        textures.push_back(loadTexture(path));
    } catch (const std::exception &e) {
        // like an unreadable mesh: a texture that cannot be read is a scene that cannot be rendered
        std::cout << "ERROR: " << e.what() << " - aborting!" << std::endl;
        throw;
    }
    return (int)textures.size() - 1;
}

Scene::~Scene() {}

int Scene::loadMaterial(std::string materialid) {
    if (atoi(materialid.c_str()) != (int)materials.size()) {
        std::cout << "ERROR: MATERIAL ID does not match expected number of materials" << std::endl;
        return -1;
    }
    if (verbose) std::cout << "Loading Material " << materials.size() << "..." << std::endl;
    Material m;
    m.specular.exponent = m.hasReflective = m.hasRefractive = m.indexOfRefraction = m.emittance = 0.0f;
    std::string line;
    for (int i = 0; i < 7; ++i) {
        safeGetline(fp_in, line);
        const Tokens t = tokenizeString(line);
        if (key(t, "RGB")) m.color = triple(t);
        else if (key(t, "SPECEX")) m.specular.exponent = num(t, 1);
        else if (key(t, "SPECRGB")) m.specular.color = triple(t);
        else if (key(t, "REFL")) m.hasReflective = num(t, 1);
        else if (key(t, "REFR")) m.hasRefractive = num(t, 1);
        else if (key(t, "REFRIOR")) m.indexOfRefraction = num(t, 1);
        else if (key(t, "EMITTANCE")) m.emittance = num(t, 1);
    }
    materials.push_back(m);
    return 1;
}

int Scene::loadCamera() {
    if (verbose) std::cout << "Loading Camera ..." << std::endl;
    Camera &camera = state.camera;
    float fovy = 0;
    std::string line;
    for (int i = 0; i < 5; ++i) {
        safeGetline(fp_in, line);
        const Tokens t = tokenizeString(line);
        if (key(t, "RES") && t.size() >= 3) {
            camera.resolution.x = atoi(t[1].c_str());
            camera.resolution.y = atoi(t[2].c_str());
        } else if (key(t, "FOVY")) fovy = num(t, 1);
        else if (key(t, "ITERATIONS") && t.size() >= 2) state.iterations = atoi(t[1].c_str());
        else if (key(t, "DEPTH") && t.size() >= 2) state.traceDepth = atoi(t[1].c_str());
        else if (key(t, "FILE") && t.size() >= 2) state.imageName = t[1];
    }
    for (safeGetline(fp_in, line); !line.empty() && fp_in.good(); safeGetline(fp_in, line)) {
        const Tokens t = tokenizeString(line);
        if (key(t, "EYE")) camera.position = triple(t);
        else if (key(t, "VIEW")) camera.view = triple(t);
        else if (key(t, "UP")) camera.up = triple(t);
    }
    deriveFov(camera, fovy);
    state.image.assign((size_t)camera.resolution.x * camera.resolution.y, lin::vec3());
    if (verbose) std::cout << "Loaded camera!" << std::endl;
    return 1;
}

int Scene::loadGeom(std::string objectid) {
    if (atoi(objectid.c_str()) != (int)geoms.size()) {
        std::cout << "ERROR: OBJECT ID does not match expected number of geoms" << std::endl;
        return -1;
    }
    if (verbose) std::cout << "Loading Geom " << geoms.size() << "..." << std::endl;
    Geom g;
    g.type = SPHERE;
    g.materialid = 0;
    std::string line;
    safeGetline(fp_in, line);
    if (!line.empty() && fp_in.good()) {
        if (line == "sphere") {
            if (verbose) std::cout << "Creating new sphere..." << std::endl;
            g.type = SPHERE;
        } else if (line == "cube") {
            if (verbose) std::cout << "Creating new cube..." << std::endl;
            g.type = CUBE;
        } else {
            const Tokens t = tokenizeString(line);
            if (t.size() >= 2 && t[0] == "mesh") {
                Mesh m;
                m.geom = (int)geoms.size();
                const std::string path = t[1][0] == '/' ? t[1] : dir + t[1];
                if (loadObj(path, m.tris, m.normals, m.mats, m.uvs) && !m.tris.empty()) {
                    if (verbose) std::cout << "Creating new mesh (" << m.tris.size() / 9 << " triangles)..." << std::endl;
                    g.type = MESH;
                    meshes.push_back(m);
                } else {
                    // a mesh that cannot be read is a scene that cannot be rendered -- not a unit sphere with the mesh's
                    // transform and material: fail the load like an unreadable scene file does
                    std::cout << "ERROR: cannot read triangles from " << path << " - aborting!" << std::endl;
                    throw std::runtime_error("cannot read triangles from " + path);
                }
            }
        }
    }
    safeGetline(fp_in, line);
    if (!line.empty() && fp_in.good()) {
        const Tokens t = tokenizeString(line);
        if (t.size() >= 2) g.materialid = atoi(t[1].c_str());
        if (verbose) std::cout << "Connecting Geom " << objectid << " to Material " << g.materialid << "..." << std::endl;
    }
    for (safeGetline(fp_in, line); !line.empty() && fp_in.good(); safeGetline(fp_in, line)) {
        const Tokens t = tokenizeString(line);
        if (key(t, "TRANS")) g.translation = triple(t);
        else if (key(t, "ROTAT")) g.rotation = triple(t);
        else if (key(t, "SCALE")) g.scale = triple(t);
        else if (key(t, "TRANS_END") || key(t, "ROTAT_END") || key(t, "SCALE_END")) {
            poseEnds.resize(geoms.size() + 1);
            PoseEnd &e = poseEnds[geoms.size()];
            if (t[0][0] == 'T') { e.trans = true; e.t = triple(t); }
            else if (t[0][0] == 'R') { e.rotat = true; e.r = triple(t); }
            else { e.scale = true; e.s = triple(t); }
        }
        else if (key(t, "TEXTURE") && t.size() >= 2) {
            const int k = textureIndex(t[1][0] == '/' ? t[1] : dir + t[1]);
            geomTextures.resize(geoms.size() + 1, -1);
            geomTextures[geoms.size()] = k;
        }
        else if (key(t, "BUMP") && t.size() >= 2) {
            char *end = nullptr;
            const float s = t.size() >= 3 ? strtof(t[2].c_str(), &end) : 0.0f;
            if (t.size() < 3 || !end || *end != 0 || !std::isfinite(s)) {
                std::cout << "ERROR: object " << objectid << ": BUMP needs a file and a finite scale - aborting!" << std::endl;
                throw std::runtime_error("BUMP without a finite scale");
            }
            const int k = textureIndex(t[1][0] == '/' ? t[1] : dir + t[1]);
            geomBumps.resize(geoms.size() + 1, -1);
            bumpScales.resize(geoms.size() + 1, 0.0f);
            geomBumps[geoms.size()] = k;
            bumpScales[geoms.size()] = s;
        }
    }
    g.transform = utilityCore::buildTransformationMatrix(g.translation, g.rotation, g.scale);
    g.inverseTransform = lin::inverse(g.transform);
    g.invTranspose = lin::inverseTranspose(g.transform);
    geoms.push_back(g);
    return 1;
}

void Scene::setResolution(int w, int h) {
    state.camera.resolution.x = w;
    state.camera.resolution.y = h;
    deriveFov(state.camera, state.camera.fov.y);
    state.image.assign((size_t)w * h, lin::vec3());
}
