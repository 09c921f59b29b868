// Stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer over the camera rays' work list as pt_init and the camera
// move build it (csrc/pt_host_scene.h: camera_list_groups, camera_list_faces_host, camera_list_emit, and build_camera_list, which puts
// the three together): host code only, no device, nothing loaded into an interpreter.  tests/run_camera_list_sanitizer.sh compiles it
// with -fsanitize=address,undefined and runs it over the pose family of tests/camera_poses.py, which that script dumps to a file:
//     int32 records, then per record: PtCamera, int32 ngeoms, PtGeom[ngeoms]
// For every record and the shards (0, 1) and (1, 3): the two passes with the host's certificates between them, without a length cap, with
// the cap at the unsplit length (the split is dropped where it does not fit) and with a cap the list does not fit; each against
// build_camera_list's arrays, element for element.  Exit status 0 and "sanitizer run finished" when clean.
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

bool same(const CameraList &a, const CameraList &b) {
    return a.pix == b.pix && a.wave == b.wave && a.sigIdx == b.sigIdx && a.face == b.face && a.nSig == b.nSig && a.listed == b.listed && a.resolved == b.resolved;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s POSES.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t records = 0;
    if (fread(&records, sizeof records, 1, f) != 1 || records < 1) { fprintf(stderr, "bad file\n"); return 2; }
    long long lists = 0, lanes = 0, resolved = 0, refused = 0, dropped = 0;
    for (int r = 0; r < records; ++r) {
        PtCamera cam;
        int32_t ngeoms = 0;
        if (fread(&cam, sizeof cam, 1, f) != 1 || fread(&ngeoms, sizeof ngeoms, 1, f) != 1 || ngeoms < 1 || ngeoms > 4096) { fprintf(stderr, "bad record %d\n", r); return 2; }
        std::vector<PtGeom> geoms((size_t)ngeoms);
        if (fread(geoms.data(), sizeof(PtGeom), (size_t)ngeoms, f) != (size_t)ngeoms) { fprintf(stderr, "short record %d\n", r); return 2; }
        KParams k;
        memset(&k, 0, sizeof k);
        camera_params(cam, k);
        k.ngeoms = ngeoms;
        magic_divisor((uint32_t)k.W, k.magicW, k.shiftW);
        std::vector<GeomDev> hg((size_t)ngeoms);
        for (int i = 0; i < ngeoms; ++i) pack_geom(geoms[(size_t)i], hg[(size_t)i], k.pos);
        CameraCull cc;
        build_camera_cull(geoms.data(), ngeoms, k, false, std::vector<const float *>((size_t)ngeoms, nullptr), hg, cc);
        CameraResolve cr;
        build_camera_resolve(geoms.data(), ngeoms, k, hg, cr);
        const int shards[2][2] = {{0, 1}, {1, 3}};
        for (const auto &sh : shards) {
            CameraGroups G0;
            const long long noCap = std::numeric_limits<long long>::max();
            if (!camera_list_groups(cc, k.W, k.H, sh[0], sh[1], noCap, G0)) { ++refused; continue; }
            const long long caps[3] = {noCap, G0.len, G0.len > 0 ? G0.len - 1 : 0};
            for (long long cap : caps) {
                for (int withFaces = 0; withFaces < 2; ++withFaces) {
                    CameraList one, two;
                    const bool built = build_camera_list(cc, k.W, k.H, sh[0], sh[1], cap, one, withFaces ? &cr : nullptr);
                    CameraGroups G;
                    const bool fits = camera_list_groups(cc, k.W, k.H, sh[0], sh[1], cap, G);
                    if (fits != built) { fprintf(stderr, "record %d: the passes and build_camera_list disagree on the cap\n", r); return 1; }
                    if (!fits) { ++refused; continue; }
                    if (withFaces) camera_list_faces_host(G, cr);
                    camera_list_emit(G, cap, two, withFaces ? &cr : nullptr);
                    if (!same(one, two)) { fprintf(stderr, "record %d: the two passes differ from build_camera_list\n", r); return 1; }
                    if (two.pix.size() % kBlock || two.wave.size() != two.pix.size() / 32 || two.face.size() != two.pix.size() / 64 || (long long)two.pix.size() > cap) {
                        fprintf(stderr, "record %d: sizes\n", r);
                        return 1;
                    }
                    for (size_t w = 0; w < two.face.size(); ++w)
                        if (two.face[w] < -1 || two.face[w] > 5 || two.wave[2 * w] < 0 || two.wave[2 * w + 1] > (int)two.sigIdx.size() || two.wave[2 * w] > two.wave[2 * w + 1]) {
                            fprintf(stderr, "record %d: wave %zu\n", r, w);
                            return 1;
                        }
                    if (withFaces && cap != noCap && two.resolved == 0 && G0.len > 0) ++dropped;
                    ++lists; lanes += (long long)two.pix.size(); resolved += two.resolved;
                }
            }
        }
    }
    fclose(f);
    printf("%d poses: %lld lists built in two passes equal build_camera_list's (%lld lanes, %lld resolved pixels, %lld capped lists without a resolved wave), %lld refused by the cap\n",
           (int)records, lists, lanes, resolved, dropped, refused);
    printf("sanitizer run finished\n");
    return 0;
}
