// keep_renderer_host.cpp -- measurements only (profiles/keep_renderer_cost.py builds and runs it): a host on the reference's three symbols,
// linked with host/pathtrace_shim.cpp, libpt_host.so and libpt_amd.so like pt_render.
//   keep_renderer_host move SCENE W H AHEAD N
//       the camera move as the reference's host makes it -- pathtraceFree(); pathtraceInit(scene); (src/main.cpp:91-95) -- by the host's
//       clock, over a renderer that has rendered 8 iterations, the eye alternating between two places; PT_AMD_TRACE_AHEAD=AHEAD.  In one
//       process, in turns: a move with the keep switch off (Free frees, Init builds), an unmeasured move that switches it on (the first
//       flagged Init finds an unflagged renderer: the full call), a move with it on (Free parks, Init moves in place).  Prints N times of
//       each kind in ms.  Built with -DPT_PARENT_SHIM against a shim without the switch: the first kind alone.
//   keep_renderer_host rate SCENE W H TEMPORAL CALLS
//       the rate of pathtrace(NULL, 0, iter) calls, iter = 1, 2, ..., after 40 unmeasured ones; TEMPORAL 1: pathtraceTemporal(true).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pathtrace.h"

#ifdef PT_PARENT_SHIM
static void pathtraceKeepRenderer(bool) {}
static void pathtraceTemporal(bool) {}
#endif

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s move SCENE W H AHEAD N | rate SCENE W H TEMPORAL CALLS\n", argv[0]); return 2; }
    Scene *scene = new Scene(argv[2]);
    scene->setResolution(atoi(argv[3]), atoi(argv[4]));
    if (!strcmp(argv[1], "rate")) {
        const int calls = atoi(argv[6]);
        pathtraceTemporal(atoi(argv[5]) != 0);
        pathtraceFree();
        pathtraceInit(scene);
        int iter = 0;
        for (int i = 0; i < 40; ++i) pathtrace(NULL, 0, ++iter);
        const double t0 = now_ms();
        for (int i = 0; i < calls; ++i) pathtrace(NULL, 0, ++iter);
        const double ms = now_ms() - t0;
        pathtraceFree();
        printf("rate %d calls %.3f ms %.1f calls/s\n", calls, ms, calls / ms * 1e3);
        return 0;
    }
    setenv("PT_AMD_TRACE_AHEAD", argv[5], 1);
    const int n = atoi(argv[6]);
    const float eyes[2][3] = {{0.0f, 5.0f, 10.5f}, {0.4f, 5.1f, 10.3f}};
    std::vector<double> without, keep;
    int moves = 0;
    const auto view = [&](bool timed, std::vector<double> *into) {
        Camera &cam = scene->state.camera;
        const float *e = eyes[moves++ % 2];
        cam.position.x = e[0]; cam.position.y = e[1]; cam.position.z = e[2];
        const double t0 = now_ms();
        pathtraceFree();
        pathtraceInit(scene);
        const double ms = now_ms() - t0;
        if (timed) into->push_back(ms);
        for (int it = 1; it <= 8; ++it) pathtrace(NULL, 0, it);
    };
    pathtraceKeepRenderer(false);
    view(false, NULL);
    view(false, NULL);
    for (int k = 0; k < n; ++k) {
        view(true, &without);
#ifndef PT_PARENT_SHIM
        pathtraceKeepRenderer(true);
        view(false, NULL);
        view(true, &keep);
        pathtraceKeepRenderer(false);
#endif
    }
    pathtraceFree();
    printf("without");
    for (double v : without) printf(" %.4f", v);
    printf("\nkeep");
    for (double v : keep) printf(" %.4f", v);
    printf("\n");
    return 0;
}
