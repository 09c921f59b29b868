"""What PT_FLAG_OBJECT_HISTORY costs on the device (profiles/object_history_cost.txt).  Cornell with its sphere moved by 0.5 along x.

  1. k_temporal<kTemporalFilter, false, true> against the MOTION = false form of the same build -- and, with --parent-test-lib, against the
     parent commit's k_temporal<kTemporalFilter> -- over the renderer's own accumulators, guides, captured history and table (pt_test_temporal_motion
     / pt_test_temporal: HIP events), 1280 x 720 and 1920 x 1080, the forms alternating, best of 35 with the median beside it.
  2. A displayed frame with history at batch 1 (pt_iterate, then pt_readback_rgba8 under PT_FLAG_DISPLAY_FILTER -- the display's bytes
     brought to the host, which synchronises --, host clock around the two calls): flagged with the moved sphere against PT_FLAG_TEMPORAL with the same scene change (the broken promise), alternating.
  3. pt_init over a live renderer with and without the flag (host clock): the extras are the scene comparison and the table.  Best of 11,
     alternating.
  --trace: nothing measured -- a flagged renderer re-initialised with NOTHING moved filters two frames, for a kernel-trace run that lists the
  kernel names: no MOTION form may appear.

    python3 profiles/object_history_cost.py [--parent-test-lib PATH] [--trace]
"""
import argparse
import ctypes as C
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

F = np.float32
DEPTH = 8


def scene_pair(pt, orc, w, h):
    import temporal_motion_ref as tm
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(w, h)
    old = np.array(sc.geoms, copy=True)
    t = old["translation"][6]
    new = tm.moved_geoms(orc, old, {6: ((float(t[0]) + 0.5, float(t[1]), float(t[2])), None, None)})
    ns = types.SimpleNamespace(geoms=old, materials=np.array(sc.materials, copy=True), camera=sc.camera.copy(), traceDepth=DEPTH, meshes={},
                               mesh_normals={}, mesh_materials={}, image=np.zeros((h, w, 3), F))
    return ns, old, new


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "best %.4f ms, median %.4f ms" % (ms[0], np.median(ms))


def kernel_cost(pt, orc, w, h, parent):
    import temporal_ref as tr
    ns, old, new = scene_pair(pt, orc, w, h)
    with pt.renderer_from_test_library():
        pt.pathtraceFree()
        ns.geoms = old
        pt.pathtraceInit(ns, traceDepth=DEPTH, moments=True, temporal=True, object_history=True, max_batch=8)
        pt.pathtrace_batch(None, 0, 1, 4)
        ns.geoms = new
        pt.pathtraceInit(ns, traceDepth=DEPTH, moments=True, temporal=True, object_history=True, max_batch=8)
        pt.pathtrace_batch(None, 0, 5, 2)
        hist = pt.test_history()
        S, Q = pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)
        pos_t, nrm_id = tr.pack_guides(*pt.gbuffer(1), h, w)
        pt.pathtraceFree()
    args = (w, h, 2, S, Q, pos_t, nrm_id, hist["hc"], hist["hn"], hist["hpos_t"], hist["hnrm_id"], hist["cam"])
    ids = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    t = {"motion": [], "plain": [], "parent": []}
    for _ in range(35):
        t["plain"].append(float(pt.test_temporal_motion(0, False, False, *args, timing_reps=1)[1][0]))
        t["motion"].append(float(pt.test_temporal_motion(0, False, True, *args, rows=hist["motion"], hist_cap=hist["cap"], timing_reps=1)[1][0]))
        if parent is not None:
            t["parent"].append(parent_temporal(parent, *args))
    print("%d x %d, %d of %d pixels on the moved sphere: k_temporal<kTemporalFilter> MOTION %s | MOTION = false %s%s" % (
        w, h, int((ids == 6).sum()), w * h, stats(t["motion"]), stats(t["plain"]), " | parent %s" % stats(t["parent"]) if parent is not None else ""))


def parent_temporal(lib, w, h, n, S, Q, pos, nrm, hc, hn, hpos, hnrm, cam):
    f = lambda a, k: np.ascontiguousarray(a, F).reshape(w * h * k)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    arrs = [f(S, 3), f(Q, 1), f(pos, 4), f(nrm, 4), f(hc, 4), f(hn, 1), f(hpos, 4), f(hnrm, 4), np.ascontiguousarray(cam, F)]
    out, out_n, ms = np.empty((w * h, 4), F), np.empty(w * h, F), np.zeros(1, F)
    lib.pt_test_temporal.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 11 + [C.c_int32, C.c_void_p]
    rc = lib.pt_test_temporal(0, w, h, n, *[p(a) for a in arrs], p(out), p(out_n), 1, p(ms))
    if rc:
        raise RuntimeError("parent pt_test_temporal: %d" % rc)
    return float(ms[0])


def display_and_init_cost(pt, orc, w, h):
    ns, old, new = scene_pair(pt, orc, w, h)
    frame = {True: [], False: []}
    init = {True: [], False: []}
    for _ in range(11):
        for flagged in (False, True):
            kind = dict(moments=True, temporal=True, object_history=flagged, display_filter=True, max_batch=1)
            pt.pathtraceFree()
            ns.geoms = old
            pt.pathtraceInit(ns, traceDepth=DEPTH, **kind)
            pt.pathtrace(None, 0, 1, readback=False)
            pt.pathtrace(None, 0, 2, readback=False)
            pt.sync()
            ns.geoms = new
            t0 = time.perf_counter()
            pt.pathtraceInit(ns, traceDepth=DEPTH, **kind)
            init[flagged].append((time.perf_counter() - t0) * 1e3)
            pt.pathtrace(None, 0, 1, readback=False)
            pt.readback_rgba8(1, w * h)
            for n in (2, 3, 4):
                t0 = time.perf_counter()
                pt.pathtrace(None, 0, n, readback=False)
                pt.readback_rgba8(n, w * h)
                frame[flagged].append((time.perf_counter() - t0) * 1e3)
    pt.pathtraceFree()
    print("%d x %d, a displayed frame with history at batch 1 (trace, commit, filter, bytes to the host): flagged, sphere followed %s | PT_FLAG_TEMPORAL %s" % (
        w, h, stats(frame[True]), stats(frame[False])))
    print("%d x %d, pt_init over a live renderer (capture included): flagged %s | PT_FLAG_TEMPORAL %s" % (w, h, stats(init[True]), stats(init[False])))


def trace_run(pt, orc):
    ns, old, _ = scene_pair(pt, orc, 320, 180)
    pt.pathtraceFree()
    pt.pathtraceInit(ns, traceDepth=DEPTH, moments=True, temporal=True, object_history=True, spatial_variance=True, max_batch=4)
    pt.pathtrace_batch(None, 0, 1, 4)
    ns.camera["position"][0] = (0.3, 5.0, 10.5)
    ns.geoms = old.copy()
    pt.pathtraceInit(ns, traceDepth=DEPTH, moments=True, temporal=True, object_history=True, spatial_variance=True, max_batch=4)
    pt.pathtrace_batch(None, 0, 5, 1)
    pt.denoise_var(1)
    pt.pathtrace_batch(None, 0, 6, 1)
    pt.denoise_var(2)
    pt.pathtraceInit(ns, traceDepth=DEPTH, moments=True, temporal=True, object_history=True, spatial_variance=True, max_batch=4)      # a capture
    pt.pathtraceFree()
    print("trace run done: a flagged renderer, nothing moved, two filtered frames and two captures")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-test-lib", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    pt = ge.load_package()
    import oracle as orc
    if a.trace:
        return trace_run(pt, orc)
    parent = C.CDLL(a.parent_test_lib) if a.parent_test_lib else None
    for w, h in ((1280, 720), (1920, 1080)):
        kernel_cost(pt, orc, w, h, parent)
    for w, h in ((1280, 720),):
        display_and_init_cost(pt, orc, w, h)


if __name__ == "__main__":
    main()
