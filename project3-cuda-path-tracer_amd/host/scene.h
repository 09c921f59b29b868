// scene.h -- the reference's `Scene` (src/scene.h:13-26): text scene file -> geoms, materials, state.
#pragma once
#include <fstream>
#include <string>
#include <vector>

#include "sceneStructs.h"
#include "utilities.h"

// (tells pathtrace_shim.cpp that this Scene has `meshes`; the reference's own scene.h, which the shim also builds against, has not)
#define PT_SCENE_HAS_MESHES 1
// (... and `textures`, `geomTextures` and Mesh::uvs: image textures bound to objects by a `TEXTURE <file>` line of their OBJECT block)
#define PT_SCENE_HAS_TEXTURES 1
// (... and `geomBumps`, `bumpScales`: height maps bound to objects by a `BUMP <file> <scale>` line of their OBJECT block)
#define PT_SCENE_HAS_BUMPS 1
// (... and `stepGeoms`: object motion across the shutter, by TRANS_END / ROTAT_END / SCALE_END lines of an OBJECT block)
#define PT_SCENE_HAS_MOTION 1

// Triangles of one `mesh` object (README.md:112-116, 236), in the OBJ file's coordinates = the geom's object space.
struct Mesh {
    int geom;                   // index into Scene::geoms (a Geom of type MESH)
    std::vector<float> tris;    // 9 floats per triangle: v0, v1, v2
    std::vector<float> normals; // 9 floats per triangle: the vertex normals n0, n1, n2 (`vn`, smooth shading) -- or EMPTY: flat shading
    std::vector<int> mats;      // one per triangle: the scene material of that face (`usemtl <k>`), -1 = the object's own -- or EMPTY
    std::vector<float> uvs;     // 6 floats per triangle: the corner texture coordinates u0 v0 u1 v1 u2 v2 (`vt`) -- or EMPTY
};

// An image texture (`TEXTURE <file>`): PPM (P3 / P6, 8 bits: texel = byte / 255, no sRGB decoding) or PFM (PF / Pf, float).  Linear RGB,
// row 0 = the image's top row.
struct Texture {
    std::string path;           // as resolved against the scene file's directory: objects naming the same file share the texture
    int width = 0, height = 0;
    std::vector<float> rgb;     // width * height * 3
};
// Reads a PPM or PFM file; throws std::runtime_error when it cannot.
Texture loadTexture(const std::string &path);

class Scene {
private:
    std::ifstream fp_in;                          // the scene file while it is being parsed
    int loadMaterial(std::string materialid);     // MATERIAL block: exactly 7 keyword lines
    int loadGeom(std::string objectid);           // OBJECT block: type, material, TRANS/ROTAT/SCALE up to a blank line
    int textureIndex(const std::string &path);    // index of the texture file `path` in `textures`, loaded at its first mention
    int loadCamera();                             // CAMERA block: 5 keyword lines + EYE/VIEW/UP up to a blank line
    bool verbose;
    std::string dir;                              // directory of the scene file ("" or ending in '/'): mesh paths are relative to it
    struct PoseEnd { bool trans = false, rotat = false, scale = false; lin::vec3 t, r, s; };
    std::vector<PoseEnd> poseEnds;                // per geom, while parsing: the *_END lines of its block
    void buildStepGeoms();                        // stepGeoms from geoms and poseEnds

public:
    // Throws std::runtime_error when the file cannot be opened (the reference prints
    // "Error reading from file - aborting!" and terminates, src/scene.cpp:12-15).
    explicit Scene(std::string filename, bool verbose = false);
    ~Scene();

    // RES override used by the headless driver; recomputes fov.x like src/scene.cpp:133-136
    void setResolution(int w, int h);

    std::vector<Geom> geoms;            // in file order = intersection order (first geom wins distance ties)
    std::vector<Material> materials;    // indexed by Geom::materialid
    std::vector<Mesh> meshes;           // one per Geom of type MESH, file order
    std::vector<Texture> textures;      // every texture file the scene names, once, in order of first mention
    std::vector<int> geomTextures;      // per geom: index into textures, or -1 (untextured)
    std::vector<int> geomBumps;         // per geom: index into textures of its height map, or -1 (unbumped)
    std::vector<float> bumpScales;      // per geom: the height map's scale (0 where unbumped)
    // Object motion (include/pt_amd.h, "motion blur"): EMPTY unless an OBJECT block carries TRANS_END, ROTAT_END or SCALE_END, else
    // kMotionSteps x geoms.size() records, step-major: step s is the scene at shutter time (s + 0.5) / kMotionSteps, every component
    // a + (b - a) * t in float between its value and its *_END value (a missing one: the component does not move), the matrices built from
    // the interpolated values as loadGeom builds them -- byte for byte the geoms of a static scene file with those values.  `geoms` keeps
    // the pose at shutter open, which is all the reference's loader reads of such a file.
    static const int kMotionSteps = 16;
    std::vector<Geom> stepGeoms;
    bool hasMotion() const { return !stepGeoms.empty(); }
    RenderState state;                  // camera, iteration count, depth, output name, host image
};
