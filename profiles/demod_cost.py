"""What albedo demodulation (PT_FLAG_DEMODULATE) costs on one MI355X, on Cornell and on scenes/cornell_textured.txt at 1280x720 and 1920x1080,
each figure against its yardstick from the same build and the same run, the two alternating, HIP events, best (median) of 35:

  iterate   pt_iterate_batch of a flagged renderer against an unflagged one, at batch 1 and at batch 64, ms per iteration: the events bracket
            the call on the renderer's stream, so the difference is what k_albedo adds to an iteration (its launch runs behind the commit)
  filter    k_demodulate (pt_test_demodulate over the device's own four-sample frame) and the last level of the shipped setting, AtrousDemod's
            of a flagged renderer against AtrousGuided's of an unflagged one (pt_test_denoise_var's per-kernel times)
  display   the displayed frame, pt_iterate_batch(.., rgba8_dev) under PT_FLAG_DISPLAY_FILTER, flagged against unflagged, ms per call at batch 1

Every step runs in a child process of its own under a time limit; the first failure ends the run, nothing is retried.

    python profiles/demod_cost.py

Prints profiles/demod_cost.txt."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES = [(1280, 720), (1920, 1080)]
SCENES = ["cornell.txt", "cornell_textured.txt"]
N = 35
STEP_LIMIT = 150        # seconds per child


def _package(scene, w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", scene))
    sc.set_resolution(w, h)
    return pt, sc


def _fmt(v, per=1.0):
    v = np.sort(np.asarray(v, np.float64)) / per
    return "%.4f (%.4f)" % (v[0], v[len(v) // 2])


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def iterate(scene, w, h, display=False):
    """two contexts, one flagged and one not, each continuing its own sequence of iterations; a measurement is one call"""
    import torch
    pt, sc = _package(scene, w, h)
    pbo = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda") if display else None
    lines = []
    for batch in ((1,) if display else (1, 64)):
        ctx = {f: pt.Context() for f in (False, True)}
        t = {False: [], True: []}
        nxt = {False: 1, True: 1}
        try:
            for f, c in ctx.items():
                with c:
                    pt.pathtraceInit(sc, max_batch=batch, moments=True, display_filter=display, demodulate=f)
            for rnd in range(N + 3):
                for f, c in ctx.items():
                    with c:
                        dt = _timed(lambda: pt.pathtrace_batch(pbo.data_ptr() if display else None, 0, nxt[f], batch))
                        nxt[f] += batch
                        if rnd >= 3:                              # (the first three rounds warm up; the display's first call makes the guides)
                            t[f].append(dt)
        finally:
            for c in ctx.values():
                with c:
                    pt.pathtraceFree()
                c.destroy()
        what = "displayed frame, pt_iterate_batch(.., rgba8_dev) at batch 1, ms per call" if display else "pt_iterate_batch at batch %2d, ms per iteration" % batch
        lines.append("  %-76s unflagged %s  flagged %s  +%.4f (+%.4f)" % (what, _fmt(t[False], batch), _fmt(t[True], batch), (min(t[True]) - min(t[False])) / batch,
                                                                           (np.median(t[True]) - np.median(t[False])) / batch))
    return lines


def filter_(scene, w, h):
    import temporal_ref as tr
    pt, sc = _package(scene, w, h)
    L = pt.PT_DISPLAY_LEVELS
    t = {"guided": [], "demod": [], "k": []}
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, max_batch=4, moments=True, demodulate=True)
        pt.pathtrace_batch(None, 0, 1, 4)
        S, Q, A = pt.readback(w * h), pt.readback_moments(), pt.test_albedo()
        g = tr.pack_guides(*pt.gbuffer(1), h, w)
        for rnd in range(5):
            r = pt.test_demodulate(1, w, h, 4, 1, A, g[0], g[1], rgb_sum=S, lum_sq_sum=Q, timing_reps=7)
            t["k"] += list(r["ms"][:, 0])
        for rnd in range(N + 2):
            for f in (False, True):
                pt.pathtraceFree()
                pt.pathtraceInit(sc, max_batch=4, moments=True, demodulate=f)
                pt.pathtrace_batch(None, 0, 1, 4)
                pt.test_denoise_var(4, 0, L)                      # (the guides, and a warm-up)
                ms = pt.test_denoise_var(4, 0, L, timing=True)[2]
                if rnd >= 2:
                    t["demod" if f else "guided"].append(ms[L])
    return ["  k_demodulate<false> (from the accumulators), ms                                                        %s" % _fmt(t["k"]),
            "  the last level (step 16, the gather): k_atrous_gather<AtrousGuided> %s  <AtrousDemod> %s  +%.4f (+%.4f)"
            % (_fmt(t["guided"]), _fmt(t["demod"]), min(t["demod"]) - min(t["guided"]), np.median(t["demod"]) - np.median(t["guided"]))]


STEPS = {"iterate": iterate, "filter": filter_, "display": lambda s, w, h: iterate(s, w, h, display=True)}

if __name__ == "__main__":
    if len(sys.argv) == 5:
        print("\n".join(STEPS[sys.argv[1]](sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        raise SystemExit(0)
    print("ms, best (median) of %d; + : flagged - unflagged, best - best (median - median)." % N, flush=True)
    for scene in SCENES:
        for w, h in FRAMES:
            print("%s %dx%d" % (scene, w, h), flush=True)
            for step in STEPS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), step, scene, str(w), str(h)], timeout=STEP_LIMIT)
                if r.returncode:
                    raise SystemExit("step %s failed with %d: stopping" % (step, r.returncode))
