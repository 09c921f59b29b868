// pathtrace.h -- the reference's renderer API (its src/pathtrace.h:6-8), provided by pathtrace_shim.cpp on top of the
// C ABI in include/pt_amd.h.  Same three names, argument meaning and error behaviour (message + exit(EXIT_FAILURE)).
#pragma once
#include "scene.h"

#ifndef PT_HAVE_UCHAR4
struct uchar4 { unsigned char x, y, z, w; };   // 4-byte RGBA texel; the host side needs no GPU header for it
#endif

// Uploads the scene and allocates the device state.  `scene` is borrowed until pathtraceFree(); call it again
// (after pathtraceFree) whenever the camera changed -- the accumulator restarts from zero.
void pathtraceInit(Scene *scene);

// Releases the device state.  Legal before the first pathtraceInit (the reference's driver calls it first).
void pathtraceFree();

// One iteration = 1 sample per pixel; `iteration` is 1-based and increasing, `frame` is always 0.
// `pbo`: DEVICE pointer to W*H uchar4 (the mapped GL buffer in the reference) or NULL when headless.
// On return scene->state.image holds the un-normalised running sum (divide by `iteration` to display).
void pathtrace(uchar4 *pbo, int frame, int iteration);

// ---- not reference symbols: switches of this build, for a host that wants them (each has an environment variable for a host that cannot call it)
// The next pathtraceInit also keeps per-pixel history across camera moves (PT_FLAG_MOMENTS | PT_FLAG_TEMPORAL, include/pt_amd.h; with
// demodulation the history carries the albedo): the variance-guided filter blends the last view's samples in.  Such a renderer traces
// nothing ahead of the pathtrace calls.  History passes a pathtraceFree only together with pathtraceKeepRenderer.  PT_AMD_TEMPORAL=1.
void pathtraceTemporal(bool on);
// pathtraceFree() PARKS the renderer instead of freeing it, and the next pathtraceInit moves its camera in place where the scene is the same
// (PT_FLAG_KEEP_RENDERER, include/pt_amd.h): the same images, a fraction of the restart's cost.  A parked renderer HOLDS ITS DEVICE MEMORY
// between Free and Init -- path pools, accumulators, tables, streams and events; only the page-locked registration of state.image is released.
// It is freed by a pathtraceFree() called while it is parked, by a pathtraceFree() after the switch was turned off, and at exit.
// PT_AMD_KEEP_RENDERER=1 (the variable, where set, decides: 0 switches it off).
void pathtraceKeepRenderer(bool on);
// Where pathtraceTemporal is on, the next pathtraceInit also sets PT_FLAG_OBJECT_HISTORY (include/pt_amd.h): a pathtraceInit whose scene shows
// the same objects in other poses keeps the history and reprojects it through each object's own motion; any other change of the scene drops
// it.  PT_AMD_OBJECT_HISTORY=1.
void pathtraceObjectHistory(bool on);
